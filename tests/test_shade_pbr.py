"""`dirt_amd.shading.shade_gbuffer_pbr` (dirt_shade_pbr.hip) and `dirt_amd.lighting.cook_torrance` against the restatement of
tests/shade_pbr_reference.py: the lighting function composed on the CPU in float64, gradients by torch's autograd.  Every
comparison is per element, |gpu - ref64| <= tol * (L1 mass of the element's terms); an element of zero mass must equal the
reference exactly; the channels of d gbuffer no attribute uses must be exact zeros.

The tolerances are measured, not chosen: the float32 torch composition is run on `tolerance_cases()`, the random inputs of
the tests below, and its worst |f32 - ref64| / mass per kind of result is F32; the kernel, which may order a pixel's sums
differently, gets 4 x that.  Produced by

    python -m tests.shade_pbr_reference

The hand-made kink pixels compare against the float32 composition on the same input by the same rule: the bound there is
KERNEL x F32 of the float64 masses as well.
"""
import ctypes
import importlib.util
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import shade_pbr_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# worst |f32 - ref64| / mass of the float32 composition on tolerance_cases(), per kind of result (python -m tests.shade_pbr_reference)
F32 = {'pixels': 1.23e-6, 'd_colors': 1.23e-6, 'd_material': 1.48e-6, 'd_normals': 2.83e-6, 'd_positions': 1.67e-6, 'd_mask': 5.95e-7,
       'd_params': 5.64e-7}
KERNEL = 4          # the kernel's allowance over the float32 composition
SENSITIVITY = 3.0e4   # test_mistakes_show_in_the_reference: the least (movement / bound) over the mistakes and kinds, recorded

MIN_ROUGHNESS, DIELECTRIC_F0 = 0.04, 0.04
NARROW = (0.25, 0.625)   # float32 numbers: an edge that float32 rounds would be an error of the comparison, not of the composition
CHANNEL_LAYOUTS = {   # name -> (Cg, layout); every channel no attribute uses holds noise
    'c11': (11, dict(colors=0, material=3, normals=5, positions=8, mask=None)),
    'c12': (12, dict(mask=0, positions=1, colors=4, normals=7, material=10)),      # examples/deferred.py and the material behind it
    'c17': (17, dict(material=0, normals=3, positions=8, mask=12, colors=14)),     # colours in the last three channels
    'c255': (255, dict(colors=100, material=253, normals=250, positions=10, mask=50)),
    'c256': (256, dict(colors=253, material=0, normals=100, positions=200, mask=252)),
    'c257': (257, dict(colors=10, material=255, normals=252, positions=30, mask=100)),     # the material crosses channel 256, in the last two
    'c1024': (1024, dict(colors=254, material=1022, normals=1000, positions=500, mask=1021)),   # the colours cross channel 256; the material last
}
TENSOR_LAYOUTS = {    # colours and material are tensors: the G-buffer needs neither
    't6': (6, dict(normals=0, positions=3, mask=None)),
    't7': (7, dict(mask=0, normals=1, positions=4)),
}
MIXED_LAYOUTS = {
    'tc': (9, dict(material=0, normals=2, positions=5, mask=8)),      # the colours a tensor, the material channels
    'ct': (10, dict(mask=0, colors=1, normals=4, positions=7)),       # the colours channels, the material a tensor
}
LAYOUTS = dict(CHANNEL_LAYOUTS, **TENSOR_LAYOUTS, **MIXED_LAYOUTS)
D, P = 'directional', 'point'


def kernel_constants():
    source = open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_shade_pbr.hip')).read()
    return tuple(int(re.search(r'constexpr int %s = (\d+);' % name, source).group(1)) for name in ('PBR_BLOCK', 'PBR_ITER'))


PBR_BLOCK, PBR_ITER = kernel_constants()
SPAN = PBR_BLOCK * PBR_ITER    # pixels of one backward workgroup
FLAT = SPAN + 3                # one full workgroup and a second with three pixels: the reduce adds two rows


class Case:
    """Inputs of one comparison: pixels that stay off the kinks, lights, ambient, camera, background, grad_out."""

    def __init__(self, seed, layout='c12', n=FLAT, kinds=(D, P), clamp=(0., 1.), mask=True, batch=None, per_scene='shared',
                 min_roughness=MIN_ROUGHNESS, dielectric_f0=DIELECTRIC_F0):
        self.cg, lay = LAYOUTS[layout]
        self.layout = dict(lay)
        if not mask:
            self.layout['mask'] = None
        self.batch, self.per_scene, self.kinds = batch, per_scene, tuple(kinds)
        self.n = n * (batch or 1)      # n: the pixels of one scene
        self.idx = np.repeat(np.arange(batch), n) if batch and per_scene != 'shared' else None
        for attempt in range(3):     # a seed that misses draw_off_kinks' cap is replaced by seed + 50, + 100 (REPLACED_SEEDS)
            rng = np.random.default_rng(seed + 50 * attempt)
            rows = batch if self.idx is not None else None
            lights = R.random_lights(rng, kinds, rows)
            shape = (rows, 3) if rows else (3,)
            self.params = {'ambient': rng.uniform(0.05, 0.3, shape), 'background': rng.uniform(0.1, 0.9, shape),
                           'camera_position': np.asarray([0.3, -0.2, 4.]) + 0.1 * rng.standard_normal(shape)}
            for i, (_, vector, color) in enumerate(lights):
                self.params['light%d.vector' % i], self.params['light%d.color' % i] = vector, color
            if per_scene == 'mixed':     # the ambient light and the lights' vectors per scene, the rest shared
                self.params = {k: v if k == 'ambient' or k.endswith('.vector') else v[0] for k, v in self.params.items()}
            self.params = {k: np.asarray(v, np.float32) for k, v in self.params.items()}
            self.lights = [(kind, self.params['light%d.vector' % i], self.params['light%d.color' % i]) for i, kind in enumerate(kinds)]
            self.kw = dict(ambient=self.params['ambient'], camera_position=self.params['camera_position'], background=self.params['background'],
                           clamp=clamp, min_roughness=min_roughness, dielectric_f0=dielectric_f0)
            try:
                self.g, self.colors, self.material, self.share = R.draw_off_kinks(rng, self.n, self.cg, self.layout, self.lights, self.kw,
                                                                                  scene_index=self.idx)
            except AssertionError:
                continue
            self.seed = seed + 50 * attempt
            break
        else:
            raise AssertionError('seed %d: no draw under the cap' % seed)
        self.go = rng.standard_normal((self.n, 3)).astype(np.float32)

    def measure(self, **more):
        return (self.g, self.lights, self.layout), dict(self.kw, colors=self.colors, material=self.material, grad_out=self.go,
                                                        scene_index=self.idx, **more)

    def reference(self, **more):
        args, kw = self.measure(**more)
        return R.compose(*args, **kw)


LIGHT_SETS = {'0': (), '1_directional': (D,), '1_point': (P,), '2_directional': (D, D), '2_point': (P, P), '2_mixed': (P, D),
              '3_directional': (D, D, D), '3_point': (P, P, P), '3_mixed': (D, P, D), '4_directional': (D, D, D, D), '4_point': (P, P, P, P),
              '4_mixed': (D, P, P, D)}
SOURCES = {'channels': 'c12', 'tensors': 't7', 'colors_tensor': 'tc', 'material_tensor': 'ct'}


def _options():
    """the four source combinations x with and without a mask x clamp set, None and narrow; the light count goes round 1..4, and
    every fourth case has a min_roughness that clamps a part of the pixels and another dielectric_f0"""
    cases, i = {}, 0
    for source, layout in SOURCES.items():
        for mask in (True, False):
            for cname, clamp in (('clamp', (0., 1.)), ('noclamp', None), ('narrow', NARROW)):
                cases['%s-%s-%s' % (source, 'mask' if mask else 'nomask', cname)] = dict(
                    seed=6100 + i, layout=layout, mask=mask, clamp=clamp, kinds=(D, P, D, P)[:1 + i % 4],
                    min_roughness=0.3 if i % 4 == 1 else MIN_ROUGHNESS, dielectric_f0=0.08 if i % 4 == 1 else DIELECTRIC_F0)
                i += 1
    return cases


def _layout_n(name):
    return FLAT if LAYOUTS[name][0] < 255 else PBR_BLOCK + 3     # the wide ones: a full pass of the copy-out walk and three pixels


CASES = dict(
    {'lights_' + name: dict(seed=6000 + i, kinds=kinds) for i, (name, kinds) in enumerate(LIGHT_SETS.items())},
    **{'pattern_channels': dict(seed=6050, layout='c12'), 'pattern_tensors': dict(seed=6051, layout='t7', kinds=(P, D, D)),
       'pattern_tensors_0': dict(seed=6053, layout='t7', kinds=())},     # tests/test_shade_pbr_edges.py: no light, both tensors
    **_options(),
    **{name: dict(seed=6200 + i, layout=name, n=_layout_n(name), kinds=(D, P, P, D)[:1 + i % 4], clamp=(0., 1.) if i % 3 else None)
       for i, name in enumerate(list(CHANNEL_LAYOUTS) + list(TENSOR_LAYOUTS))},
    **{'scenes_%d_%s' % (n, per): dict(seed=6300 + 3 * i + j, layout=('c12', 't7', 'tc')[j], n=n, batch=3, per_scene=per, kinds=(P, D)[:1 + i])
       for i, n in enumerate((SPAN, SPAN + 1)) for j, per in enumerate(('shared', 'per_scene', 'mixed'))})
REPLACED_SEEDS = {}     # case -> the seed it ended with, where that is not the one above (DESIGN.md §7b names them)
_CASES = {}


def case_of(name):
    if name not in _CASES:
        case = Case(**CASES[name])
        _CASES[name] = (case, case.reference())
    return _CASES[name]


def tolerance_cases():
    return {name: Case(**kw) for name, kw in CASES.items()}


# ---- the fused call

def shade(case, dev, want=(True, True, True, True), g=None, colors=None, material=None):
    """-> dict of the fused call's results on `case`: out and the gradients wanted of (G-buffer, parameters, colour tensor,
    material tensor); `colors` / `material`: tensors to use in place of the case's"""
    from dirt_amd import shading
    want_g, want_p, want_c, want_m = want
    shape = (case.batch, case.n // case.batch, 1) if case.batch else (case.n,)
    g = torch.from_numpy(case.g).to(dev).reshape(shape + (case.cg,)) if g is None else g
    g = g.detach().requires_grad_(want_g)
    prm = {k: torch.from_numpy(v).to(dev).requires_grad_(want_p) for k, v in case.params.items()}
    col, mat = case.layout.get('colors'), case.layout.get('material')
    if col is None:
        col = (torch.from_numpy(case.colors).to(dev).reshape(shape + (3,)) if colors is None else colors).detach().requires_grad_(want_c)
    if mat is None:
        mat = (torch.from_numpy(case.material).to(dev).reshape(shape + (2,)) if material is None else material).detach().requires_grad_(want_m)
    lights = [(kind, prm['light%d.vector' % i], prm['light%d.color' % i]) for i, kind in enumerate(case.kinds)]
    out = shading.shade_gbuffer_pbr(g, lights, colors=col, material=mat, normals=case.layout['normals'], positions=case.layout['positions'],
                                    mask=case.layout.get('mask'), ambient=prm['ambient'], camera_position=prm['camera_position'],
                                    background=prm['background'], clamp=case.kw['clamp'], min_roughness=case.kw['min_roughness'],
                                    dielectric_f0=case.kw['dielectric_f0'])
    res = {'out': out.detach().reshape(-1, 3)}
    if out.requires_grad:
        out.backward(torch.from_numpy(case.go).to(dev).reshape(out.shape))
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
    return res


def check(case, got, ref, what, factor=KERNEL):
    """The mass rule per kind of result, exact equality where the mass is zero, exact zeros in the unused channels."""
    worst = R.ratios(got, ref)
    print(what, ' '.join('%s %.2f' % (k, v / F32[k]) for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= factor * F32[k], '%s %s: |gpu - ref64| / mass = %.3e, allowed %.3e' % (what, k, v, factor * F32[k])
    triples = [(got.get(key), ref.get(key), ref.get(mass)) for _, key, mass in R.PAIRS]
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


def compare(name, dev, want=(True, True, True, True)):
    case, ref = case_of(name)
    got = shade(case, dev, want)
    check(case, got, ref, name)
    return case, ref, got


# ---- CPU tests

def _numpy_ct(p, n, c, r, mu, cam, lights, min_roughness=0.04, f0=0.04):
    """the specification of DESIGN.md §7b written out in numpy float64; p, n, c [..., V, 3], r, mu [..., V], cam and the lights'
    vectors and colours [..., 3]"""
    nrm = lambda x: x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-12)   # noqa: E731
    dot = lambda a, b: (a * b).sum(-1, keepdims=True)   # noqa: E731
    N, v = nrm(n), nrm(cam[..., None, :] - p)
    rho = np.clip(r, min_roughness, 1.)[..., None]
    mu = mu[..., None]
    a2, k = (rho ** 2) ** 2, (rho + 1.) ** 2 / 8.
    F0 = f0 * (1. - mu) + c * mu
    nv = np.maximum(dot(N, v), 0.)
    total = np.zeros_like(p)
    for kind, d, col in lights:
        l = nrm(-d[..., None, :]) + 0. * p if kind == 'directional' else nrm(d[..., None, :] - p)
        h = nrm(l + v)
        nl, nh, vh = np.maximum(dot(N, l), 0.), np.maximum(dot(N, h), 0.), np.maximum(dot(v, h), 0.)
        x = np.cross(N, h)
        den = dot(x, x) + a2 * nh ** 2
        Dg = a2 / (np.pi * den ** 2)
        vis = 0.25 / ((nl * (1. - k) + k) * (nv * (1. - k) + k))
        F = F0 + (1. - F0) * (1. - vh) ** 5
        kd = (1. - F) * (1. - mu)
        total = total + (kd * c / np.pi + Dg * vis * F) * col[..., None, :] * nl
    return total


def test_cook_torrance_against_the_specification():
    from dirt_amd import lighting
    rng = np.random.default_rng(6400)
    t = torch.from_numpy
    for batch in ((), (2,)):
        p, n, c = rng.uniform(-1., 1., batch + (7, 3)), rng.standard_normal(batch + (7, 3)), rng.uniform(0., 1., batch + (7, 3))
        r, mu = rng.uniform(0., 1.2, batch + (7,)), rng.uniform(0., 1., batch + (7,))
        cam = np.asarray([0.3, -0.2, 4.]) + 0.1 * rng.standard_normal(batch + (3,))
        lights = [(D, rng.standard_normal(batch + (3,)), rng.uniform(0., 1., batch + (3,))),
                  (P, 3. * rng.standard_normal(batch + (3,)), rng.uniform(0., 1., batch + (3,)))]
        for used in (lights, lights[:1], lights[1:], []):
            for mr, f0 in ((0.04, 0.04), (0.5, 0.1)):
                want = _numpy_ct(p, n, c, r, mu, cam, used, mr, f0)
                got = lighting.cook_torrance(t(p), t(n), t(c), t(r), t(mu), t(cam), [(k, t(d), t(col)) for k, d, col in used], mr, f0)
                assert got.shape == batch + (7, 3) and got.dtype == torch.float64
                assert np.abs(got.numpy() - want).max() <= 1e-13 * max(1., np.abs(want).max())
    for kw, text in ((dict(min_roughness=0.), 'min_roughness must be > 0 and <= 1, got 0.0'),
                     (dict(min_roughness=1.5), 'min_roughness must be > 0 and <= 1, got 1.5'),
                     (dict(dielectric_f0=-0.1), 'dielectric_f0 must lie in [0, 1], got -0.1'),
                     (dict(dielectric_f0=1.1), 'dielectric_f0 must lie in [0, 1], got 1.1')):
        with pytest.raises(ValueError) as e:
            lighting.cook_torrance(t(p), t(n), t(c), t(r), t(mu), t(cam), [], **kw)
        assert str(e.value) == text
    with pytest.raises(ValueError, match="light 0: expected"):
        lighting.cook_torrance(t(p), t(n), t(c), t(r), t(mu), t(cam), [('spot', t(cam), t(cam))])
    # the restatement's value is the specification's
    case = Case(seed=6401, n=64, kinds=(D, P))
    ref = case.reference(masses=False)
    lay = case.layout
    g = case.g.astype(np.float64)
    sl = lambda k, w: g[:, None, lay[k]:lay[k] + w]   # noqa: E731
    f64 = lambda x: np.asarray(x, np.float64)   # noqa: E731
    lit = _numpy_ct(sl('positions', 3), sl('normals', 3), sl('colors', 3), g[:, None, lay['material']], g[:, None, lay['material'] + 1],
                    f64(case.params['camera_position'])[None], [(k, f64(d)[None], f64(c)[None]) for k, d, c in case.lights])[:, 0]
    m = g[:, lay['mask']:lay['mask'] + 1]
    pre = (f64(case.params['ambient']) * g[:, lay['colors']:lay['colors'] + 3] + lit) * m + f64(case.params['background']) * (1. - m)
    assert np.abs(ref['pre'].numpy() - pre).max() <= 1e-12


def _aligned(cos_theta, roughness, color=(1., 1., 1.), metalness=1.):
    """camera and light along +z, the normal tilted by theta: n . l = n . v = n . h = cos(theta), v . h = 1 -> the lobes"""
    from dirt_amd import lighting
    t = np.asarray(cos_theta, np.float64)
    n = torch.from_numpy(np.stack([np.sqrt(1. - t * t), 0. * t, t], -1))
    one = torch.ones(len(t), dtype=torch.float64)
    return lighting.cook_torrance_lobes(torch.zeros(len(t), 3, dtype=torch.float64), n, torch.tensor(color, dtype=torch.float64).expand(len(t), 3),
                                        roughness * one, metalness * one, torch.tensor([0., 0., 5.], dtype=torch.float64),
                                        [(D, torch.tensor([0., 0., -1.], dtype=torch.float64), torch.ones(3, dtype=torch.float64))])[0]


def test_the_distribution_integrates_to_one():
    """int D (n . h) d omega = 1 over the hemisphere, by 400-node Gauss-Legendre in cos(theta), for roughness 0.25, 0.5 and 1
    (below 0.25 the peak outruns the nodes).  D is read off the specular lobe of a white metal seen along the light, where
    F = 1 and Vis is known: D = specular / Vis."""
    t, wt = np.polynomial.legendre.leggauss(400)
    t, wt = 0.5 * (t + 1.), 0.5 * wt      # [0, 1]
    for roughness in (0.25, 0.5, 1.):
        _, specular, weight, products = _aligned(t, roughness)
        k = (roughness + 1.) ** 2 / 8.
        vis = 0.25 / (t * (1. - k) + k) ** 2
        Dg = specular[:, 0].numpy() / vis
        assert np.abs(weight[:, 0].numpy() - t).max() <= 1e-15 and np.abs(products.sum(-1).numpy() - t).max() <= 1e-15
        assert abs(2. * np.pi * (Dg * t * wt).sum() - 1.) <= 1e-10, roughness


def test_limit_cases():
    from dirt_amd import lighting
    t = np.linspace(0.05, 1., 20)
    # a metal has no diffuse lobe, exactly
    diffuse, specular, _, _ = _aligned(t, 0.5, color=(0.9, 0.5, 0.2), metalness=1.)
    assert not bool(diffuse.any()) and bool((specular > 0).all())
    # v . h = 1: the Fresnel term is F0, so the specular lobe is D Vis F0
    f0 = 0.04 * (1. - 0.3) + np.asarray([0.9, 0.5, 0.2]) * 0.3
    _, specular, _, _ = _aligned(t, 0.5, color=(0.9, 0.5, 0.2), metalness=0.3)
    a2, k = 0.5 ** 4, 1.5 ** 2 / 8.
    want = (a2 / (np.pi * ((1. - t * t) + a2 * t * t) ** 2) * 0.25 / (t * (1. - k) + k) ** 2)[:, None] * f0
    assert np.abs(specular.numpy() - want).max() <= 1e-13 * want.max()
    # a light behind the surface contributes exactly 0, whatever the lobes are
    rng = np.random.default_rng(6402)
    n = torch.from_numpy(rng.standard_normal((50, 3)))
    d = torch.tensor([0.3, -0.5, 0.8], dtype=torch.float64)
    behind = (n * -d).sum(-1) < 0
    args = (torch.from_numpy(rng.uniform(-1., 1., (50, 3))), n, torch.from_numpy(rng.uniform(0., 1., (50, 3))), torch.from_numpy(rng.uniform(0., 1., 50)),
            torch.from_numpy(rng.uniform(0., 1., 50)), torch.tensor([0., 0., 4.], dtype=torch.float64))
    lit = lighting.cook_torrance(*args, [(D, d, torch.ones(3, dtype=torch.float64))])
    assert 5 < int(behind.sum()) < 45 and not bool(lit[behind].any()) and bool((lit[~behind] > 0).all())
    assert not bool(lighting.cook_torrance(*args, []).any())


def test_the_float32_composition_stays_within_the_committed_figures():
    """F32 is what `python -m tests.shade_pbr_reference` prints: measured again here on every case of this file (Case asserts
    draw_off_kinks' cap: under 5 % of a first draw rejected)."""
    worst = dict.fromkeys(R.KINDS, 0.)
    for name in CASES:
        case, _ = case_of(name)
        assert case.share < 0.05, name
        assert REPLACED_SEEDS.get(name, CASES[name]['seed']) == case.seed, (name, case.seed)
        measured = R.measure_f32([case.measure()])
        for k, v in measured.items():
            assert v <= F32[k], '%s %s: committed %.3e, measured on this case %.3e' % (name, k, F32[k], v)
            worst[k] = max(worst[k], v)
    print({k: '%.3e' % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v >= 0.5 * F32[k], '%s: committed %.3e is not what these inputs give (%.3e)' % (k, F32[k], v)
        assert F32[k] <= 1e-5, k


def test_the_cases_hold_what_their_names_say():
    assert (PBR_BLOCK, PBR_ITER) == (256, 4) and FLAT == 1027
    header = open(os.path.join(ROOT, 'include', 'dirt_hip.h')).read()
    assert '#define DIRT_SHADE_MAX_CHANNELS 1024' in header and '#define DIRT_SHADE_PBR_MAX_LIGHTS 4' in header
    for name, kinds in LIGHT_SETS.items():
        case, ref = case_of('lights_' + name)
        assert case.kinds == kinds and len(kinds) == int(name[0]) and case.n == FLAT and ref['cosines'].shape == (FLAT, 1 + 3 * len(kinds))
        assert ('mixed' in name) == (len(set(kinds)) == 2) and (name.endswith('point')) == (set(kinds) == {P})
    assert sorted(len(k) for k in LIGHT_SETS.values()) == [0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4]
    for name in LAYOUTS:
        cg, lay = LAYOUTS[name]
        used = sorted(ch for k, w in R.ATTRIBUTES if lay.get(k) is not None for ch in range(lay[k], lay[k] + w))
        assert len(set(used)) == len(used) and used[-1] < cg, name
    for name in list(CHANNEL_LAYOUTS) + list(TENSOR_LAYOUTS):
        case, _ = case_of(name)
        assert case.g.shape == (case.n, LAYOUTS[name][0]) and (case.colors is None) == (name in CHANNEL_LAYOUTS) == (case.material is None)
    assert sorted(LAYOUTS[k][0] for k in CHANNEL_LAYOUTS) == [11, 12, 17, 255, 256, 257, 1024] and sorted(LAYOUTS[k][0] for k in TENSOR_LAYOUTS) == [6, 7]
    for source, (col, mat) in (('channels', (False, False)), ('tensors', (True, True)), ('colors_tensor', (True, False)), ('material_tensor', (False, True))):
        case, ref = case_of(source + '-mask-clamp')
        assert (case.colors is not None, case.material is not None) == (col, mat)
        assert case_of(source + '-nomask-narrow')[0].layout['mask'] is None
    case, ref = case_of('channels-mask-narrow')
    inside = float(((ref['pre'] > NARROW[0]) & (ref['pre'] < NARROW[1])).double().mean())
    assert 0.1 < inside < 0.9, inside
    case, ref = case_of('colors_tensor-mask-noclamp')      # i = 13: min_roughness 0.3 clamps a share of the pixels
    assert case.kw['min_roughness'] == 0.3 and 0.02 < float((ref['roughness'] < 0.3).double().mean()) < 0.2
    assert case_of('scenes_%d_per_scene' % SPAN)[0].params['light0.vector'].shape == (3, 3)
    mixed = case_of('scenes_%d_mixed' % (SPAN + 1))[0]
    assert mixed.n == 3 * (SPAN + 1) and mixed.params['ambient'].shape == (3, 3) and mixed.params['light1.color'].shape == (3,)
    assert case_of('scenes_%d_shared' % SPAN)[0].idx is None
    dark, ref = case_of('pattern_tensors_0')
    assert dark.kinds == () and dark.colors is not None and dark.material is not None and dark.n == FLAT and ref['cosines'].shape == (FLAT, 1)


def _movement(alt, ref, kinds):
    """the worst (|alt - ref| / mass) / bound per kind of result"""
    moved = R.ratios(alt, ref)
    return {k: moved[k] / (KERNEL * F32[k]) for k in kinds}


def test_mistakes_show_in_the_reference():
    """On the restatement alone: a light's specular lobe dropped, its diffuse lobe dropped, two scenes' parameter rows swapped,
    roughness and metalness swapped -- each moves some element of every kind of result it can affect by more than 100 x its
    bound, so a kernel with that mistake could not pass.  SENSITIVITY records the least factor."""
    case, ref = case_of('scenes_%d_per_scene' % (SPAN + 1))
    args, kw = case.measure(masses=False)
    kinds = [k for k in R.KINDS if k != 'd_colors' and k != 'd_material'] + ['d_colors', 'd_material']     # t7: both are tensors
    factors = {}
    for light in range(len(case.kinds)):
        for lobe in ('specular', 'diffuse'):
            factors['%s %d' % (lobe, light)] = _movement(R.compose(*args, **dict(kw, drop=(light, lobe))), ref, kinds)
    swapped = {k: v[[1, 0, 2]] for k, v in case.params.items()}
    lights = [(kind, swapped['light%d.vector' % i], swapped['light%d.color' % i]) for i, kind in enumerate(case.kinds)]
    alt = R.compose(args[0], lights, args[2], **dict(kw, ambient=swapped['ambient'], camera_position=swapped['camera_position'],
                                                     background=swapped['background']))
    factors['rows swapped'] = _movement(alt, ref, kinds)
    factors['material swapped'] = _movement(R.compose(*args, **dict(kw, swap_material=True)), ref, kinds)
    least = min(v for f in factors.values() for v in f.values())
    print('least factor %.3g' % least, {m: min(f, key=f.get) for m, f in factors.items()})
    for mistake, f in factors.items():
        for k, v in f.items():
            assert v > 100, (mistake, k, v)
    assert 0.5 * SENSITIVITY <= least <= 2. * SENSITIVITY, least


G = torch.zeros(4, 5, 12)
CPU = ' runs on an MI355X only; there is no CPU fallback'


def test_shade_gbuffer_pbr_refuses_bad_arguments():
    from dirt_amd import _lib, shading
    light = shading.pbr_directional_light((0., 0., -1.), (1., 1., 1.))
    assert light == ('directional', (0., 0., -1.), (1., 1., 1.)) and shading.pbr_point_light((1., 2., 3.), (1., 1., 1.))[0] == 'point'

    def check_args(g=G, lights=(light,), colors=4, material=10, normals=7, positions=1, mask=0, ambient=(0., 0., 0.), camera_position=(0., 0., 4.),
                   background=(0., 0., 0.), clamp=(0., 1.), min_roughness=0.04, dielectric_f0=0.04):
        return shading._check_pbr_arguments(g, list(lights), colors, material, normals, positions, mask, ambient, camera_position, background, clamp,
                                            min_roughness, dielectric_f0)

    G4 = torch.zeros(2, 4, 5, 12)
    for kw, text in (
            (dict(g=G.to(torch.int32)), 'shade_gbuffer_pbr expects a float32 gbuffer, got torch.int32'),
            (dict(colors=torch.zeros(4, 5, 4)), "colors as a tensor must have shape [4, 5, 3] (the G-buffer's [4, 5, 12] with 3 channels), got [4, 5, 4]"),
            (dict(colors=torch.zeros(4, 5, 3, dtype=torch.int64)), 'colors as a tensor must be floating-point, got torch.int64'),
            (dict(colors=torch.zeros(4, 5, 3, device='meta')), 'colors is on meta, the G-buffer on cpu'),
            (dict(material=torch.zeros(4, 5, 3)), "material as a tensor must have shape [4, 5, 2] (the G-buffer's [4, 5, 12] with 2 channels), got [4, 5, 3]"),
            (dict(material=torch.zeros(4, 5, 2, dtype=torch.int32)), 'material as a tensor must be floating-point, got torch.int32'),
            (dict(material=torch.zeros(4, 5, 2, device='meta')), 'material is on meta, the G-buffer on cpu'),
            (dict(material=None), 'material must be the index of a G-buffer channel, got None'),
            (dict(material=11), 'material at channel 11 does not fit in the 12 channels of the G-buffer'),
            (dict(material=6), 'material (channel 6) overlaps colors (channel 4)'),
            (dict(normals=9), 'normals (channel 9) overlaps material (channel 10)'),
            (dict(positions=None), 'positions must be the index of a G-buffer channel, got None'),
            (dict(positions=5), 'positions (channel 5) overlaps colors (channel 4)'),
            (dict(mask=3), 'mask (channel 3) overlaps positions (channel 1)'),
            (dict(colors=1.5), 'colors must be the index of a G-buffer channel, got 1.5'),
            (dict(lights=[light] * 5), 'shade_gbuffer_pbr takes at most 4 lights, got 5'),
            (dict(lights=[('spot', (0., 0., 1.), (1., 1., 1.))]),
             "light 0: expected a record starting with one of ['directional', 'point'], got ('spot', (0.0, 0.0, 1.0), (1.0, 1.0, 1.0))"),
            (dict(lights=[light, ('point', (0., 0., 1.))]), 'light 1: a point record has 3 fields, got 2'),
            (dict(lights=[('point', (0., 1.), (1., 1., 1.))]), 'light 0 position must be 3 numbers, got 2'),
            (dict(lights=[('directional', torch.zeros(2, 3), (1., 1., 1.))]), 'light 0 direction must have shape [3], got [2, 3]'),
            (dict(lights=[('directional', (0., 0., 1.), torch.zeros(3, device='meta'))]), 'light 0 color is on meta, the G-buffer on cpu'),
            (dict(min_roughness=0.), 'min_roughness must be a number > 0 and <= 1, got 0.0'),
            (dict(min_roughness=1.01), 'min_roughness must be a number > 0 and <= 1, got 1.01'),
            (dict(min_roughness=torch.tensor(0.1)), 'min_roughness must be a number > 0 and <= 1, got tensor(0.1000)'),
            (dict(dielectric_f0=-0.5), 'dielectric_f0 must be a number in [0, 1], got -0.5'),
            (dict(dielectric_f0='a'), "dielectric_f0 must be a number in [0, 1], got 'a'"),
            (dict(camera_position=None), 'shade_gbuffer_pbr needs camera_position'),
            (dict(camera_position=(1., 2.)), 'camera_position must be 3 numbers, got 2'),
            (dict(ambient=torch.zeros(2, 3)), 'ambient must have shape [3], got [2, 3]'),
            (dict(background=(1., 2.)), 'background must be 3 numbers, got 2'),
            (dict(clamp=(1., 0.)), 'clamp needs lo <= hi, got (1.0, 0.0)'),
            (dict(clamp=3.), 'clamp must be (lo, hi) or None, got 3.0')):
        with pytest.raises(ValueError) as e:
            check_args(**kw)
        assert str(e.value) == text, (kw, str(e.value))
    offsets, kinds, scalars, lo, hi, flags, const, tensors = check_args(
        g=G4, lights=[light, ('point', torch.ones(2, 3), (0.5, 0.6, 0.7)), ('point', (1., 2., 3.), torch.ones(3))], ambient=(0.1, 0.2, 0.3),
        min_roughness=0.1, dielectric_f0=1)
    assert offsets == [4, 10, 7, 1, 0] and kinds == 0b110 and scalars == (0.1, 1.) and (lo, hi) == (0., 1.) and flags == _lib.SHADE_CLAMP
    assert const == [0.1, 0.2, 0.3, 0., 0., 0., 0., 0., 4.] + [0., 0., -1., 1., 1., 1., 0., 0.] + [0., 0., 0., 0.5, 0.6, 0.7, 0., 0.] + [1., 2., 3.] + [0.] * 5
    assert [(s, tuple(t.shape)) for s, t in tensors] == [(17, (2, 3)), (28, (1, 3))]
    block = shading._splice_block(G4.device, const, tensors)
    assert block.shape == (2, 33) and bool((block[:, 17:20] == 1).all()) and bool((block[:, 28:31] == 1).all()) and not bool(block[:, 31:].any())
    assert check_args(clamp=None)[3:6] == (0., 0., 0)
    assert check_args(colors=torch.zeros(4, 5, 3), material=torch.zeros(4, 5, 2), mask=None)[0] == [-1, -1, 7, 1, -1]
    assert check_args(lights=[])[1] == 0 and len(check_args(lights=[])[6]) == 9
    with pytest.raises(ValueError) as e:
        shading.shade_gbuffer_pbr(torch.zeros(5), [], colors=0, material=3, normals=5, positions=8, camera_position=(0., 0., 1.))
    assert str(e.value) == 'shade_gbuffer_pbr expects gbuffer [H, W, Cg], [B, H, W, Cg] or [N, Cg], got (5,)'
    for g in (G, G.to('meta')):
        with pytest.raises(RuntimeError) as e:
            shading.shade_gbuffer_pbr(g, [], colors=4, material=10, normals=7, positions=1, camera_position=(0., 0., 1.))
        assert str(e.value) == 'dirt_amd.shading.shade_gbuffer_pbr' + CPU
    with pytest.raises(TypeError):
        shading.shade_gbuffer_pbr(G, [], colors=4, material=10, normals=7, positions=1)      # camera_position is required


def test_the_function_is_exported_and_declared():
    import dirt
    import dirt.shading
    import dirt.lighting
    import dirt_amd
    from dirt_amd import _lib, build
    assert dirt.shading.shade_gbuffer_pbr is dirt_amd.shading.shade_gbuffer_pbr
    assert dirt.shading.pbr_directional_light is dirt_amd.shading.pbr_directional_light and dirt.shading.pbr_point_light is dirt_amd.shading.pbr_point_light
    assert dirt.lighting.cook_torrance is dirt_amd.lighting.cook_torrance
    assert 'dirt_shade_pbr.hip' in build.SOURCES and 'dirt_shade_pbr.hip' not in build.PER_SOURCE_FLAGS
    header = open(os.path.join(ROOT, 'include', 'dirt_hip.h')).read()
    for symbol in ('dirt_shade_pbr_scratch_bytes', 'dirt_shade_pbr_forward', 'dirt_shade_pbr_backward'):
        assert symbol in _lib.SYMBOLS and re.search(r'\b%s\(' % symbol, header)
    assert '#define DIRT_SHADE_PBR_MAX_LIGHTS %d\n' % _lib.SHADE_PBR_MAX_LIGHTS in header and _lib.SHADE_PBR_MAX_LIGHTS == 4
    assert _lib.SHADE_PBR_KINDS == {'directional': 0, 'point': 1} and _lib.ABI_VERSION == 4 and '#define DIRT_ABI_VERSION 4' in header
    source = open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_shade_pbr.hip')).read()
    assert 'atomicAdd' not in source and 'atomic_' not in source and 'powf' not in source


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
        d = dict(scenes=1, pixels=64, cg=12, cs=0, ms=0, oc=4, omat=10, on=7, op=1, om=0, ps=1, lights=2, kinds=2, mr=0.04, f0=0.04, lo=0., hi=1., flags=1)
        d.update(kw)
        return tuple(d[k] for k in ('scenes', 'pixels', 'cg', 'cs', 'ms', 'oc', 'omat', 'on', 'op', 'om', 'ps', 'lights', 'kinds', 'mr', 'f0', 'lo', 'hi',
                                    'flags')) + (None,)

    def fwd(g=one, c=None, m=None, p=one, out=one, **kw):
        return lib.dirt_shade_pbr_forward(g, c, m, p, out, *tail(kw))

    def bwd(g=one, c=None, m=None, p=one, go=one, gg=one, gc=None, gm=None, gp=one, scratch=one, nbytes=1 << 20, **kw):
        return lib.dirt_shade_pbr_backward(g, c, m, p, go, gg, gc, gm, gp, scratch, nbytes, *tail(kw))

    for who, call in (('dirt_shade_pbr_forward', fwd), ('dirt_shade_pbr_backward', bwd)):
        for kw, text in ((dict(cg=1025), '%s: 1025 G-buffer channels, 1..1024'), (dict(cg=0), '%s: 0 G-buffer channels, 1..1024'),
                         (dict(scenes=-1), '%s: negative sizes (scenes=-1 pixels=64)'), (dict(pixels=-5), '%s: negative sizes (scenes=1 pixels=-5)'),
                         (dict(scenes=65536), '%s: 65536 scenes, at most 65535'),
                         (dict(c=one, cs=2), '%s: color_stride=2, a pixel\'s colour is 3 floats'),
                         (dict(m=one, ms=1), '%s: material_stride=1, a pixel\'s material is 2 floats'),
                         (dict(lights=5, kinds=0), '%s: 5 lights, at most 4'), (dict(lights=-1, kinds=0), '%s: -1 lights, at most 4'),
                         (dict(lights=2, kinds=4), '%s: light_kinds 0x4 has bits beyond 2 lights'),
                         (dict(lights=0, kinds=1), '%s: light_kinds 0x1 has bits beyond 0 lights'),
                         (dict(ps=2), '%s: param_scenes=2 is neither 1 nor scenes=1'),
                         (dict(flags=3), '%s: unknown flags 0x3'), (dict(flags=4), '%s: unknown flags 0x4'),
                         (dict(oc=9), '%s: material (channel 10) overlaps colors (channel 9)'),
                         (dict(oc=-1), '%s: colors at channel -1 does not fit in 12 channels'),
                         (dict(omat=11), '%s: material at channel 11 does not fit in 12 channels'),
                         (dict(on=5), '%s: normals (channel 5) overlaps colors (channel 4)'),
                         (dict(op=9), '%s: positions (channel 9) overlaps material (channel 10)'),
                         (dict(op=-1), '%s: positions at channel -1 does not fit in 12 channels'),
                         (dict(om=3), '%s: mask (channel 3) overlaps positions (channel 1)'),
                         (dict(om=12), '%s: mask at channel 12 does not fit in 12 channels'),
                         (dict(mr=0.), '%s: min_roughness=0 is not in (0, 1]'), (dict(mr=1.5), '%s: min_roughness=1.5 is not in (0, 1]'),
                         (dict(mr=float('nan')), '%s: min_roughness=nan is not in (0, 1]'),
                         (dict(f0=-0.25), '%s: dielectric_f0=-0.25 is not in [0, 1]'), (dict(f0=2.), '%s: dielectric_f0=2 is not in [0, 1]'),
                         (dict(lo=1., hi=0.), '%s: clamp bounds lo=1 > hi=0')):
            assert call(**kw) == E, (who, kw)
            assert lib.dirt_last_error().decode() == text % who, (who, kw, lib.dirt_last_error())
        assert call(pixels=0) == 0 and call(scenes=0) == 0 and lib.dirt_last_error() == b''
        # with tensors off_colors and off_material are not read, and the G-buffer may be six channels
        assert call(c=one, cs=3, m=one, ms=2, oc=-1, omat=-1, cg=6, on=0, op=3, om=-1, pixels=0) == 0
        assert call(c=one, cs=5, m=one, ms=5, oc=7, omat=7, pixels=0) == 0
    assert fwd(out=None) == E and lib.dirt_last_error().decode() == 'dirt_shade_pbr_forward: gbuffer / params / out is NULL'
    assert fwd(g=None) == E and fwd(p=None) == E
    assert bwd(go=None) == E and lib.dirt_last_error().decode() == 'dirt_shade_pbr_backward: gbuffer / params / grad_out is NULL'
    assert bwd(gc=one) == E
    assert lib.dirt_last_error().decode() == 'dirt_shade_pbr_backward: grad_colors without colors (the channel path\'s is part of grad_gbuffer)'
    assert bwd(gm=one) == E
    assert lib.dirt_last_error().decode() == 'dirt_shade_pbr_backward: grad_material without material (the channel path\'s is part of grad_gbuffer)'
    assert bwd(gg=None, gp=None) == 0      # nothing wanted: nothing is launched
    need = lib.dirt_shade_pbr_scratch_bytes(1, 64, 2)
    assert need == 4 * 25 and lib.dirt_shade_pbr_scratch_bytes(3, FLAT, 4) == 4 * 41 * 3 * 2 and lib.dirt_shade_pbr_scratch_bytes(1, 64, 0) == 36
    for bad in ((-1, 64, 1), (65536, 64, 1), (1, -1, 1), (1, 64, 5), (1, 64, -1)):
        assert lib.dirt_shade_pbr_scratch_bytes(*bad) == 0
    assert bwd(nbytes=need - 1) == E
    assert lib.dirt_last_error().decode() == 'dirt_shade_pbr_backward: scratch is NULL or smaller than dirt_shade_pbr_scratch_bytes (99 < 100)'
    assert bwd(scratch=None) == E and bwd(scratch=ctypes.c_void_p(18)) == E and b'4-byte aligned' in lib.dirt_last_error()


def test_the_kernels_use_no_scratch_memory():
    from dirt_amd import build
    res = {k: v for k, v in build.kernel_resources().items() if 'shade_pbr_' in k}
    assert len(res) == 21, sorted(res)       # the forward and <lights 0..4, PARAMS, GBUF>
    for name, v in res.items():
        assert v['scratch'] == 0 and v['lds'] <= 16384, (name, v)


# ---- GPU tests

@pytest.mark.gpu
@pytest.mark.parametrize('name', list(LIGHT_SETS))
def test_light_sets_against_the_restatement(gpu, name):
    compare('lights_' + name, gpu)


PATTERNS = [('channels', w + (False, False)) for w in itertools.product((True, False), repeat=2)] + \
           [('tensors', w) for w in itertools.product((True, False), repeat=4)]


@pytest.mark.gpu
@pytest.mark.parametrize('path, want', PATTERNS, ids=['%s-%s' % (p, ''.join(n for n, on in zip('gpcm', w) if on) or 'none') for p, w in PATTERNS])
def test_every_pattern_of_wanted_gradients(gpu, path, want):
    """One flat frame of a workgroup's span + 3 pixels through each pattern of wanted gradients (G-buffer, parameters, colour
    tensor, material tensor), none included; what is not wanted stays absent."""
    case, ref, got = compare('pattern_' + path, gpu, want)
    assert ('d_gbuffer' in got) == want[0] and ('d_params' in got) == want[1]
    assert ('d_colors' in got) == (want[2] if path == 'tensors' else want[0]) and ('d_material' in got) == (want[3] if path == 'tensors' else want[0])
    assert ('d_normals' in got) == want[0]


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(_options()))
def test_sources_masks_and_clamps_against_the_restatement(gpu, name):
    compare(name, gpu)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CHANNEL_LAYOUTS) + list(TENSOR_LAYOUTS))
def test_layouts_against_the_restatement(gpu, name):
    compare(name, gpu)


@pytest.mark.gpu
@pytest.mark.parametrize('name', [k for k in CASES if k.startswith('scenes_')])
def test_scenes_that_end_on_and_past_a_workgroup_boundary(gpu, name):
    compare(name, gpu)


@pytest.mark.gpu
def test_strided_tensors_are_read_in_place(gpu, monkeypatch):
    """`tex[..., :3]` and `tex[..., 3:5]` of a five-channel look-up: the pointers the C ABI receives are the tensor's own at
    stride 5, and every result has the bits of the run on contiguous copies.  Both gradients are dense."""
    from dirt_amd import _stage, _lib
    case, ref = case_of('pattern_tensors')
    seen = []
    call = _stage.call
    monkeypatch.setattr(_stage, 'call', lambda f, dev, *args, **kw: (seen.append((f, args)), call(f, dev, *args, **kw))[1])
    lib = _lib.load()
    plain = shade(case, gpu)
    (forward,) = [a for f, a in seen if f is lib.dirt_shade_pbr_forward]
    assert forward[8:10] == (3, 2)
    tex = torch.full((case.n, 5), 1.e30, device=gpu)
    tex[:, :3], tex[:, 3:5] = torch.from_numpy(case.colors).to(gpu), torch.from_numpy(case.material).to(gpu)
    del seen[:]
    got = shade(case, gpu, colors=tex[:, :3], material=tex[:, 3:5])
    (forward,) = [a for f, a in seen if f is lib.dirt_shade_pbr_forward]
    (backward,) = [a for f, a in seen if f is lib.dirt_shade_pbr_backward]
    assert forward[1:3] == (tex.data_ptr(), tex.data_ptr() + 12) and forward[8:10] == (5, 5)
    assert backward[1:3] == forward[1:3] and backward[14:16] == (5, 5)
    assert got['d_colors'].is_contiguous() and got['d_material'].is_contiguous()
    check(case, got, ref, 'slices of a [N, 5] tensor')
    for k in ('out', 'd_gbuffer', 'd_colors', 'd_material'):
        assert torch.equal(got[k], plain[k]), k
    for k in plain['d_params']:
        assert torch.equal(got['d_params'][k], plain['d_params'][k]), k


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['c1024', 'scenes_%d_per_scene' % (SPAN + 1), 'lights_4_mixed'])
def test_two_runs_give_the_same_bits(gpu, name):
    case, _ = case_of(name)
    a, b = shade(case, gpu), shade(case, gpu)
    assert set(a) == set(b)
    for k in a:
        if k == 'd_params':
            assert all(torch.equal(a[k][p], b[k][p]) for p in a[k]), k
        else:
            assert torch.equal(a[k], b[k]), k


def _abi(lib, dev, case, n, guard=7):
    """forward and backward through the C ABI on the first n pixels of `case`, every output inside `guard` floats of 12345 on
    both sides -> (out, grad_gbuffer, grad_colors or None, grad_material or None, grad_params), the guards checked"""
    from dirt_amd import _lib
    g = torch.from_numpy(case.g[:n]).to(dev).contiguous()
    col = torch.from_numpy(case.colors[:n]).to(dev).contiguous() if case.colors is not None else None
    mat = torch.from_numpy(case.material[:n]).to(dev).contiguous() if case.material is not None else None
    nl = len(case.kinds)
    block = np.zeros((1, 9 + 8 * nl), np.float32)
    block[0, 0:3], block[0, 3:6], block[0, 6:9] = case.params['ambient'], case.params['background'], case.params['camera_position']
    for i in range(nl):
        block[0, 9 + 8 * i:12 + 8 * i], block[0, 12 + 8 * i:15 + 8 * i] = case.params['light%d.vector' % i], case.params['light%d.color' % i]
    block = torch.from_numpy(block).to(dev)
    go = torch.from_numpy(case.go[:n]).to(dev).contiguous()

    def guarded(count):
        t = torch.full((count + 2 * guard,), 12345., device=dev)
        return t, t[guard:guard + count]

    bufs = {k: guarded(c) for k, c in (('out', 3 * n), ('gg', case.cg * n), ('gc', 3 * n), ('gm', 2 * n), ('gp', 9 + 8 * nl))}
    lo, hi = case.kw['clamp']
    lay = case.layout
    kinds = sum(1 << i for i, kind in enumerate(case.kinds) if kind == P)
    tail = (1, n, case.cg, 3 if col is not None else 0, 2 if mat is not None else 0, lay.get('colors', -1), lay.get('material', -1), lay['normals'],
            lay['positions'], lay['mask'] if lay.get('mask') is not None else -1, 1, nl, kinds, case.kw['min_roughness'], case.kw['dielectric_f0'],
            lo, hi, _lib.SHADE_CLAMP, None)
    cp, mp = (t.data_ptr() if t is not None else None for t in (col, mat))
    nbytes = lib.dirt_shade_pbr_scratch_bytes(1, n, nl)
    sfull, scratch = guarded(nbytes // 4)
    torch.cuda.synchronize()
    _lib.check(lib.dirt_shade_pbr_forward(g.data_ptr(), cp, mp, block.data_ptr(), bufs['out'][1].data_ptr(), *tail))
    _lib.check(lib.dirt_shade_pbr_backward(g.data_ptr(), cp, mp, block.data_ptr(), go.data_ptr(), bufs['gg'][1].data_ptr(),
                                           bufs['gc'][1].data_ptr() if col is not None else None, bufs['gm'][1].data_ptr() if mat is not None else None,
                                           bufs['gp'][1].data_ptr(), scratch.data_ptr(), nbytes, *tail))
    torch.cuda.synchronize()
    for k, (full, inner) in list(bufs.items()) + [('scratch', (sfull, scratch))]:
        if (k == 'gc' and col is None) or (k == 'gm' and mat is None):
            assert bool((full == 12345.).all())
            continue
        assert bool((full[:guard] == 12345.).all()) and bool((full[-guard:] == 12345.).all()), k
        assert not bool((inner == 12345.).any()), k
    return (bufs['out'][1].reshape(n, 3), bufs['gg'][1].reshape(n, case.cg), bufs['gc'][1].reshape(n, 3) if col is not None else None,
            bufs['gm'][1].reshape(n, 2) if mat is not None else None, bufs['gp'][1])


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 255, 256, 257, FLAT])
@pytest.mark.parametrize('path', ['channels', 'tensors'])
def test_the_c_abi_writes_inside_its_outputs(gpu, lib, path, n):
    """Guard values around out, grad_gbuffer, grad_colors, grad_material, grad_params (and the scratch) stay; every element
    inside is written.  The results are the wrapper's on the whole frame (which test_every_backward_instantiation holds against
    the restatement), bit for bit: all of them at the whole frame, the first n pixels' at a shorter one (a pass of one pixel, a
    partial and a full pass, a second pass of one pixel), where a pixel's values do not depend on how many follow it."""
    case, ref = case_of('pattern_' + path)
    out, gg, gc, gm, gp = _abi(lib, gpu, case, n)
    got = shade(case, gpu)
    assert torch.equal(out, got['out'][:n]) and torch.equal(gg, got['d_gbuffer'][:n])
    assert (gc is None or torch.equal(gc, got['d_colors'][:n])) and (gm is None or torch.equal(gm, got['d_material'][:n]))
    if n == case.n:
        assert torch.equal(gp[0:3], got['d_params']['ambient']) and torch.equal(gp[3:6], got['d_params']['background'])
        assert torch.equal(gp[6:9], got['d_params']['camera_position'])
        for i in range(len(case.kinds)):
            assert torch.equal(gp[9 + 8 * i:12 + 8 * i], got['d_params']['light%d.vector' % i])
            assert torch.equal(gp[12 + 8 * i:15 + 8 * i], got['d_params']['light%d.color' % i]) and not bool(gp[15 + 8 * i:17 + 8 * i].any())


KINK_LAYOUT = dict(mask=0, colors=1, normals=4, positions=7, material=10)
KINK_KW = dict(ambient=(0.1, 0.1, 0.1), camera_position=(0.25, -0.5, 4.), background=(0.2, 0.3, 0.4), clamp=None, min_roughness=0.25, dielectric_f0=0.04)
KINK_LIGHTS = [(D, (-1., 0., 0.), (0.5, 0.5, 0.5)), (P, (1., 2., 3.), (0.25, 0.5, 0.5))]


def _pixels(dev, rows, lights=KINK_LIGHTS, kw=KINK_KW):
    """hand-made pixels [m, c[3], n[3], p[3], r, mu] through the fused call and through the float64 and float32 compositions on the same input"""
    from dirt_amd import shading
    g = np.asarray(rows, np.float32)
    go = np.ones((len(g), 3), np.float32)
    gt = torch.from_numpy(g).to(dev).requires_grad_(True)
    names = R.param_names(len(lights))
    values = [kw['ambient'], kw['background'], kw['camera_position']] + [x for rec in lights for x in rec[1:3]]
    prm = {k: torch.tensor(v, dtype=torch.float32, device=dev, requires_grad=True) for k, v in zip(names, values)}
    recs = [(rec[0], prm['light%d.vector' % i], prm['light%d.color' % i]) for i, rec in enumerate(lights)]
    out = shading.shade_gbuffer_pbr(gt, recs, ambient=prm['ambient'], background=prm['background'], camera_position=prm['camera_position'],
                                    clamp=kw['clamp'], min_roughness=kw['min_roughness'], dielectric_f0=kw['dielectric_f0'], **KINK_LAYOUT)
    out.backward(torch.from_numpy(go).to(dev))
    got = {'out': out.detach(), 'd_gbuffer': gt.grad, 'd_params': {k: v.grad for k, v in prm.items()}}
    for k, w in R.ATTRIBUTES:
        got['d_' + k] = gt.grad[:, KINK_LAYOUT[k]:KINK_LAYOUT[k] + w]
    refs = [R.compose(g, lights, KINK_LAYOUT, grad_out=go, dtype=dt, masses=dt == torch.float64, **kw) for dt in (torch.float64, torch.float32)]
    return got, refs[0], refs[1]


def _near(got, r64, r32, skip=()):
    """|gpu - f32 composition| and |gpu - ref64| within KERNEL x F32 of the float64 masses, non-finite values in the same places"""
    triples = [(kind, got[key], r64[key], r32[key], r64[mass]) for kind, key, mass in R.PAIRS if kind not in skip]
    triples += [('d_params', got['d_params'][k], r64['d_params'][k], r32['d_params'][k], r64['mass_params'][k]) for k in got['d_params']]
    for kind, a, ref64, ref32, mass in triples:
        a = a.detach().cpu().double().reshape(ref64.shape)
        for r in (ref64, ref32.double()):
            assert torch.equal(torch.isfinite(a), torch.isfinite(r)), kind
            ok = torch.isfinite(r)
            bound = KERNEL * F32[kind] * mass
            assert bool(((a - r).abs()[ok] <= bound[ok]).all()), (kind, a, r, bound)


@pytest.mark.gpu
def test_kink_a_grazing_light_passes_the_gradient(gpu):
    """n . l exactly 0 for the directional light (the normal along z, the light along -x): max(x, 0) passes the gradient at its
    edge, so d normals has the light's share although the light adds nothing to the pixel."""
    rows = [[1., 0.5, 0.25, 0.75, 0., 0., 1., 0.25, -0.5, 0.5, 0.5, 0.5], [0.5, 0.5, 0.25, 0.75, 0., 0., 2., 0., 0., 0., 0.75, 0.]]
    got, r64, r32 = _pixels(gpu, rows)
    assert bool((r64['cosines'][:, 1] == 0).all())
    _near(got, r64, r32)
    without, _, _ = _pixels(gpu, rows, KINK_LIGHTS[1:])
    assert torch.equal(torch.isfinite(got['out']), torch.isfinite(without['out']))
    assert bool(((got['out'] - without['out']).abs() <= 1e-6).all()) and bool((got['d_normals'][:, 0] != without['d_normals'][:, 0]).all())


@pytest.mark.gpu
def test_kink_roughness_outside_its_range(gpu):
    """Roughness below min_roughness (0.25 here), exactly on it, exactly 1 and above 1: the value is the clamped roughness's,
    the gradient passes at both edges and stops outside."""
    rows = [[1., 0.5, 0.25, 0.75, 0.25, 0.25, 1., 0.25, -0.5, 0.5, r, 0.5] for r in (0.125, 0.25, 0.5, 1., 1.5)]
    got, r64, r32 = _pixels(gpu, rows)
    _near(got, r64, r32)
    d_r = got['d_material'][:, 0]
    assert not bool(d_r[[0, 4]].any()) and bool((d_r[1:4] != 0).all())
    assert torch.equal(got['out'][0], got['out'][1]) and torch.equal(got['out'][3], got['out'][4])


@pytest.mark.gpu
def test_kink_metalness_zero_and_one(gpu):
    rows = [[1., 0.5, 0.25, 0.75, 0.25, 0.25, 1., 0.25, -0.5, 0.5, 0.5, mu] for mu in (0., 1.)]
    got, r64, r32 = _pixels(gpu, rows)
    _near(got, r64, r32)
    assert bool((got['d_material'][:, 1] != 0).all())


@pytest.mark.gpu
def test_kink_the_point_at_the_camera(gpu):
    """p = cam: the view vector is the zero vector (0 / max(0, 1e-12)), n . v = 0 and v . h = 0, the norm's gradient is 0 there."""
    rows = [[1., 0.5, 0.25, 0.75, 0.25, 0.25, 1., 0.25, -0.5, 4., 0.5, 0.5]]
    got, r64, r32 = _pixels(gpu, rows)
    assert bool((r64['cosines'][:, 0] == 0).all())
    _near(got, r64, r32)
    assert bool(torch.isfinite(got['d_gbuffer']).all())


@pytest.mark.gpu
def test_kink_a_zero_normal(gpu):
    """n = 0: N is the zero vector, |N x h|^2 + a2 (N . h)^2 is 0 and D is a2 / 0 -- the float32 composition gives inf * 0 for
    the lights' terms, and the kernel has its non-finite values in the same places; the pixel beside it is untouched."""
    rows = [[1., 0.5, 0.25, 0.75, 0., 0., 0., 0.25, -0.5, 0.5, 0.5, 0.5], [1., 0.5, 0.25, 0.75, 0.25, 0.25, 1., 0.25, -0.5, 0.5, 0.5, 0.5]]
    got, r64, r32 = _pixels(gpu, rows)
    alone, a64, a32 = _pixels(gpu, rows[1:])
    for k in ('out', 'd_gbuffer'):
        g32 = r32['d_gbuffer' if k == 'd_gbuffer' else k]
        assert torch.equal(torch.isfinite(got[k]).cpu(), torch.isfinite(g32)), k
        assert torch.equal(got[k][1], alone[k][0]), k
    assert not bool(torch.isfinite(got['out'][0]).any())


@pytest.mark.gpu
def test_graph_capture_replays_on_changed_inputs(gpu):
    """Forward and backward captured with torch.cuda.graph (the call makes no host synchronisation), replayed once after the
    inputs were overwritten in place: the replay has the eager bits of the new inputs."""
    from dirt_amd import shading
    case, _ = case_of('pattern_tensors')
    other = Case(seed=6052, layout='t7', kinds=case.kinds)
    eager = shade(other, gpu)
    t = lambda x: torch.from_numpy(x).to(gpu)   # noqa: E731
    g, col, mat = (t(x).requires_grad_(True) for x in (case.g, case.colors, case.material))
    prm = {k: t(v).requires_grad_(True) for k, v in case.params.items()}
    go = t(case.go)
    names = list(prm)

    def step():
        lights = [(kind, prm['light%d.vector' % i], prm['light%d.color' % i]) for i, kind in enumerate(case.kinds)]
        out = shading.shade_gbuffer_pbr(g, lights, colors=col, material=mat, normals=case.layout['normals'], positions=case.layout['positions'],
                                        mask=case.layout['mask'], ambient=prm['ambient'], camera_position=prm['camera_position'],
                                        background=prm['background'], clamp=case.kw['clamp'])
        return (out,) + torch.autograd.grad(out, [g, col, mat] + [prm[k] for k in names], go)

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
        for dst, src in [(g, other.g), (col, other.colors), (mat, other.material), (go, other.go)] + [(prm[k], other.params[k]) for k in names]:
            dst.copy_(t(src))
    for x in captured:
        x.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for x, k in zip(captured[:4], ('out', 'd_gbuffer', 'd_colors', 'd_material')):
        assert torch.equal(x.reshape(eager[k].shape), eager[k]), k
    for x, k in zip(captured[4:], names):
        assert torch.equal(x, eager['d_params'][k]), k


def _load_example(name):
    spec = importlib.util.spec_from_file_location('example_' + name, os.path.join(ROOT, 'examples', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_rasterise_deferred_with_a_texture_feeding_both_tensors(gpu):
    """The example's cube on a 32 x 24 frame through rasterise_deferred: a five-channel sample_texture_uv look-up hands
    `[..., :3]` and `[..., 3:5]` to shade_gbuffer_pbr, against the same call with the shader written with lighting.cook_torrance.
    Pixels and the light colour's gradient by the mass rule (masses from the restatement on the rasterised G-buffer and the
    looked-up texels); the texture's and the vertices' gradients come through the look-up's and the rasteriser's backward,
    where no mass is at hand: an element agrees if |a - b| <= 1e-3 max(|a|, |b|) (or both are below 1e-7); at most 1 % may not."""
    import dirt_amd
    from dirt_amd import lighting, shading, texture as tex
    ex = _load_example('fit_material_fused')
    W, H = 32, 24
    vertices_np, uvs_np, faces_np = ex.textured.build_cube()
    ambient, background = (0.05, 0.05, 0.05), (0., 0., 0.3)
    results = []
    for fused in (False, True):
        vertices = torch.from_numpy(vertices_np).to(gpu).requires_grad_(True)
        uvs, faces = torch.from_numpy(uvs_np).to(gpu), torch.from_numpy(faces_np).to(gpu)
        texture = torch.from_numpy(ex.material_texture()).to(gpu).requires_grad_(True)
        color = torch.tensor(ex.TRUE_COLOR, device=gpu, requires_grad=True)
        clip, attributes, camera = ex.geometry(vertices, uvs, faces)
        seen = {}

        def fn(gbuffer, texture_, color_):
            looked_up = tex.sample_texture_uv(texture_, gbuffer[..., 1:3])
            seen['gbuffer'], seen['texels'] = gbuffer.detach(), looked_up.detach()
            if fused:
                lights = [shading.pbr_directional_light(ex.LIGHT_DIRECTION, color_), shading.pbr_point_light(*ex.POINT_LIGHT)]
                return shading.shade_gbuffer_pbr(gbuffer, lights, colors=looked_up[..., :3], material=looked_up[..., 3:5], camera_position=camera,
                                                 ambient=ambient, background=background, **ex.LAYOUT)
            m, n, p = gbuffer[..., :1], gbuffer[..., 3:6], gbuffer[..., 6:9]
            c = looked_up[..., :3]
            as_t = lambda x: torch.tensor(x, device=gbuffer.device)   # noqa: E731
            lit = lighting.cook_torrance(p, n, c, looked_up[..., 3], looked_up[..., 4], camera,
                                         [('directional', as_t(ex.LIGHT_DIRECTION), color_), ('point', as_t(ex.POINT_LIGHT[0]), as_t(ex.POINT_LIGHT[1]))])
            return torch.clamp((as_t(ambient) * c + lit) * m + as_t(background) * (1. - m), 0., 1.)

        pixels = dirt_amd.rasterise_deferred(ex.background_attributes(H, W, gpu), clip, attributes, faces, fn, [texture, color])
        (pixels ** 2).mean().backward()
        results.append((pixels.detach(), color.grad, texture.grad, vertices.grad, seen, camera.detach()))
    (pa, ca, ta, va, _, _), (pb, cb, tb, vb, seen, camera) = results
    assert 0.1 < float((seen['gbuffer'][..., 0] > 0).float().mean()) < 0.9      # the cube covers a sixth of the frame
    go = (2. / pa.numel()) * pa.reshape(-1, 3).cpu().numpy()
    texels = seen['texels'].reshape(-1, 5).cpu().numpy()
    ref = R.compose(seen['gbuffer'].reshape(-1, 9).cpu().numpy(), [(D, ex.LIGHT_DIRECTION, ex.TRUE_COLOR), (P,) + ex.POINT_LIGHT], ex.LAYOUT,
                    colors=texels[:, :3], material=texels[:, 3:5], ambient=ambient, camera_position=camera.cpu().numpy(), background=background,
                    grad_out=go)
    for what, a, b, r, mass, f in (('pixels', pa, pb, ref['out'], ref['mass_out'], F32['pixels']),
                                   ('d light colour', ca, cb, ref['d_params']['light0.color'], ref['mass_params']['light0.color'], F32['d_params'])):
        a, b = a.cpu().double().reshape(mass.shape), b.cpu().double().reshape(mass.shape)
        for x, y, factor in ((b, r, KERNEL), (b, a, KERNEL + 1)):     # against the restatement; against the torch shader, which has its own F32
            assert bool(((x - y).abs() <= factor * f * mass).all()), (what, float(((x - y).abs() / mass.clamp_min(1e-300)).max()), f)
    for what, a, b in (('d texture', ta, tb), ('d vertices', va, vb)):
        a, b = a.cpu().double(), b.cpu().double()
        agree = ((a - b).abs() <= 1e-3 * torch.maximum(a.abs(), b.abs())) | ((a.abs() < 1e-7) & (b.abs() < 1e-7))
        print('deferred: %s: %d of %d elements excluded' % (what, int((~agree).sum()), agree.numel()))
        assert 1. - float(agree.double().mean()) <= 0.01 and bool(a.abs().max() > 0), what
    assert bool(tb[..., 3:5].abs().max() > 0)      # the material channels of the texture receive a gradient


@pytest.mark.gpu
def test_the_example_recovers_the_material(gpu):
    ex = _load_example('fit_material_fused')
    losses, before, after = ex.fit(width=64, height=48, steps=30, device=gpu)
    assert losses[-1] < losses[0] and after < before
