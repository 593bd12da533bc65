"""`dirt_amd.shading.shade_gbuffer_ibl` (dirt_shade_ibl.hip), `dirt_amd.lighting.image_based_lighting` and
`dirt_amd.lighting.environment_brdf` against the restatement of tests/shade_ibl_reference.py: the lighting function composed
on the CPU in float64, gradients by torch's autograd.  Every comparison is per element, |gpu - ref64| <= tol * (L1 mass of the
element's terms); an element of zero mass must equal the reference exactly; the channels of d gbuffer no attribute uses must
be exact zeros.

The tolerances are measured, not chosen: the float32 torch composition is run on `tolerance_cases()`, the random inputs of
the tests below, and its worst |f32 - ref64| / mass per kind of result is F32; the kernel, which may order a pixel's sums
differently, gets 4 x that.  Produced by

    python -m tests.shade_ibl_reference

The random pixels keep 1e-3 from every kink, judged by the float64 restatement alone before any kernel runs
(`shade_ibl_reference.kink_distance`): a tap-lattice line of any look-up used, in index units (pyramid levels l and l + 1,
the irradiance cube, the table); an integer lod; a roughness clamp edge; nv = 0; a face tie of R or n; an edge of the output's
clamp.  The hand-made kink pixels compare against the float32 composition on the same input by the same rule: the bound there
is KERNEL x F32 of the float64 masses as well.
"""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import shade_ibl_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# worst |f32 - ref64| / mass of the float32 composition on tolerance_cases(), per kind of result (python -m tests.shade_ibl_reference)
F32 = {'pixels': 1.27e-6, 'd_colors': 1.18e-6, 'd_material': 4.18e-5, 'd_normals': 2.21e-5, 'd_positions': 6.84e-5, 'd_mask': 1.91e-7,
       'd_params': 3.28e-7, 'd_specular': 3.68e-4, 'd_irradiance': 1.44e-5}
KERNEL = 4          # the kernel's allowance over the float32 composition
TABLE_ERROR = 1.64e-4  # the table reference's own convergence error (python -m tests.shade_ibl_reference); the table gets KERNEL x that
SENSITIVITY = 7.0e4  # test_mistakes_show_in_the_reference: the least (movement / bound) over the mistakes, recorded

LAYOUTS = {   # name -> (Cg, layout); every channel no attribute uses holds noise
    'c12': (12, dict(mask=0, positions=1, colors=4, normals=7, material=10)),
    'c257': (257, dict(colors=10, material=255, normals=252, positions=30, mask=100)),     # the material crosses channel 256, in the last two
    't6': (6, dict(normals=0, positions=3, mask=None)),                # colours and material are tensors: the G-buffer needs neither
    'tc': (9, dict(material=0, normals=2, positions=5, mask=8)),       # the colours a tensor, the material channels
    'ct': (10, dict(mask=0, colors=1, normals=4, positions=7)),        # the colours channels, the material a tensor
}
BASE_ENV = (8, 4, 4, 16)     # pyramid size and levels, irradiance size, table size
AXES = {'+x': (1., 0., 0.), '-x': (-1., 0., 0.), '+y': (0., 1., 0.), '-y': (0., -1., 0.), '+z': (0., 0., 1.), '-z': (0., 0., -1.)}
FACE = {'+x': 0, '-x': 1, '+y': 2, '-y': 3, '+z': 4, '-z': 5}


def kernel_constants():
    source = open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_shade_ibl.hip')).read()
    return tuple(int(re.search(r'constexpr int %s = (\d+);' % name, source).group(1)) for name in ('IBL_BLOCK', 'IBL_ITER'))


IBL_BLOCK, IBL_ITER = kernel_constants()
SPAN = IBL_BLOCK * IBL_ITER    # pixels of one backward workgroup
FLAT = SPAN + 3                # one full workgroup and a second with three pixels: the reduce adds two rows


def _towards(axis, spread, seed, roughness=None):
    """a case's placement: normals around `axis` (the camera sits on it, the positions near the origin), so that n and the
    mirrored view vector stay within `spread` of it; roughness: (lo, hi) to draw it from, so that lod stays inside one pair of
    levels (a G-buffer with material channels)"""
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)

    def fix(g, rows, layout):
        rng = np.random.default_rng(seed + len(rows))
        n = axis + spread * rng.standard_normal((len(rows), 3))
        g[rows, layout['normals']:layout['normals'] + 3] = n / np.linalg.norm(n, axis=1, keepdims=True) * rng.uniform(0.8, 1.2, (len(rows), 1))
        g[rows, layout['positions']:layout['positions'] + 3] = rng.uniform(-0.3, 0.3, (len(rows), 3))
        if roughness is not None:
            g[rows, layout['material']] = rng.uniform(*roughness, len(rows))
    return fix, tuple(4. * axis)


class Case:
    """Inputs of one comparison: an environment, pixels that stay off the kinks, intensity, camera, background, grad_out."""

    def __init__(self, seed, n=FLAT, layout='c12', env=BASE_ENV, batch=None, params='shared', grid=None, towards=None, clamp=(0., 1.)):
        rng = np.random.default_rng(seed)
        self.cg, self.layout = LAYOUTS[layout]
        self.batch, self.grid = batch, grid
        if grid is not None:
            n = grid[0] * grid[1]
        self.n = n * (batch or 1)
        self.env = R.Environment(rng, *env)
        self.kw = dict(clamp=clamp, min_roughness=0.04, dielectric_f0=0.04)
        rows = {'shared': (None, None, None), 'per_scene': (batch, batch, batch), 'mixed': (batch, None, batch)}[params]
        shape = lambda b: (3,) if b is None else (b, 3)   # noqa: E731
        fix, camera = None, None
        if towards is not None:
            placed, camera = _towards(towards[0], towards[1], seed, *towards[2:])
            fix = lambda g, at: placed(g, at, self.layout)   # noqa: E731
        cam = np.broadcast_to(np.asarray(camera if camera is not None else (0.25, -0.5, 4.)), shape(rows[2])) + 0.05 * rng.standard_normal(shape(rows[2]))
        self.params = {'intensity': rng.uniform(0.6, 1.0, shape(rows[0])).astype(np.float32),
                       'background': rng.uniform(0.2, 0.6, shape(rows[1])).astype(np.float32), 'camera_position': cam.astype(np.float32)}
        self.scene_index = np.repeat(np.arange(batch), n) if batch else None
        self.g, self.colors, self.material, self.share = R.draw_off_kinks(rng, self.n, self.cg, self.layout, self.env, dict(self.kw, **self.params),
                                                                          self.scene_index, fix)
        self.go = rng.standard_normal((self.n, 3)).astype(np.float32)

    def measure(self):
        return (self.g, self.env, self.layout), dict(colors=self.colors, material=self.material, grad_out=self.go, scene_index=self.scene_index,
                                                     **self.kw, **self.params)

    def reference(self):
        args, kw = self.measure()
        return R.compose(*args, **kw)


CASES = dict(
    [('pixels_%d' % n, dict(seed=7100 + n, n=n)) for n in (1, 255, 256, 257, SPAN - 1, SPAN, FLAT)] +
    [('scenes_' + p, dict(seed=7200 + i, n=IBL_BLOCK + 44, batch=3, params=p)) for i, p in enumerate(('shared', 'per_scene', 'mixed'))] +
    [('env_%d_%d_%d_%d' % e, dict(seed=7300 + i, n=300, env=e)) for i, e in enumerate(((1, 1, 1, 2), (2, 2, 5, 32), (6, 2, 4, 16), (12, 3, 5, 32), (8, 1, 4, 2)))] +
    [('layout_' + k, dict(seed=7400 + i, n=300, layout=k)) for i, k in enumerate(LAYOUTS)] +
    [('face_' + k, dict(seed=7500 + i, n=200, towards=(a, 0.08))) for i, (k, a) in enumerate(AXES.items())] +
    [('tile_one_face', dict(seed=7600, grid=(16, 16), towards=(AXES['+z'], 0.08, (0.36, 0.64)))),      # lod in (1, 2) of 4 levels
     ('tile_edge_and_corner', dict(seed=7601, grid=(16, 16), towards=((1., 1., 1.), 0.15))),
     ('image_20x37', dict(seed=7602, grid=(20, 37), batch=2, params='per_scene')),
     ('no_clamp', dict(seed=7603, n=300, clamp=None)),
     ('pattern', dict(seed=7604, n=FLAT, layout='t6'))])
_CASES = {}


def case_of(name):
    """-> (the case, its float64 reference): made once, shared by the tests, never changed"""
    if name not in _CASES:
        case = Case(**CASES[name])
        _CASES[name] = (case, case.reference())
    return _CASES[name]


def tolerance_cases():
    return {name: Case(**kw) for name, kw in CASES.items()}


# ---- the fused call

WANT_ALL = dict(gbuffer=True, params=True, colors=True, material=True, specular=True, irradiance=True)


def shade(case, dev, want=WANT_ALL, colors=None, material=None):
    """-> dict of the fused call's results on `case`: out and the gradients wanted; `colors` / `material`: tensors to use in
    place of the case's"""
    from dirt_amd import shading, texture
    want = dict(dict.fromkeys(WANT_ALL, False), **want)
    shape = ((case.batch,) if case.batch else ()) + (case.grid if case.grid else (case.n // (case.batch or 1),) + ((1,) if case.batch else ()))
    g = torch.from_numpy(case.g).to(dev).reshape(shape + (case.cg,)).requires_grad_(want['gbuffer'])
    prm = {k: torch.from_numpy(v).to(dev).requires_grad_(want['params']) for k, v in case.params.items()}
    col, mat = case.layout.get('colors'), case.layout.get('material')
    if col is None:
        col = (torch.from_numpy(case.colors).to(dev).reshape(shape + (3,)) if colors is None else colors).detach().requires_grad_(want['colors'])
    if mat is None:
        mat = (torch.from_numpy(case.material).to(dev).reshape(shape + (2,)) if material is None else material).detach().requires_grad_(want['material'])
    env = case.env
    levels = len(env.levels)
    packed = torch.from_numpy(env.packed()).to(dev).requires_grad_(want['specular'])
    pyramid = texture.CubePyramid(packed, env.size, 3, levels, tuple(k / (levels - 1) for k in range(levels)) if levels > 1 else (0.,))
    irr = torch.from_numpy(env.irradiance).to(dev).requires_grad_(want['irradiance'])
    out = shading.shade_gbuffer_ibl(g, pyramid, irr, torch.from_numpy(env.table).to(dev), colors=col, material=mat, normals=case.layout['normals'],
                                    positions=case.layout['positions'], mask=case.layout.get('mask'), intensity=prm['intensity'],
                                    camera_position=prm['camera_position'], background=prm['background'], clamp=case.kw['clamp'],
                                    min_roughness=case.kw['min_roughness'], dielectric_f0=case.kw['dielectric_f0'])
    res = {'out': out.detach().reshape(-1, 3)}
    if out.requires_grad:
        out.backward(torch.from_numpy(case.go).to(dev).reshape(out.shape))
    if want['gbuffer']:
        res['d_gbuffer'] = g.grad.reshape(-1, case.cg)
        for k, w in R.ATTRIBUTES:
            if case.layout.get(k) is not None:
                res['d_' + k] = res['d_gbuffer'][:, case.layout[k]:case.layout[k] + w]
    if isinstance(col, torch.Tensor) and want['colors']:
        res['d_colors'] = col.grad.reshape(-1, 3)
    if isinstance(mat, torch.Tensor) and want['material']:
        res['d_material'] = mat.grad.reshape(-1, 2)
    if want['params']:
        res['d_params'] = {k: v.grad for k, v in prm.items()}
    if want['specular']:
        res['d_specular'] = packed.grad
    if want['irradiance']:
        res['d_irradiance'] = irr.grad
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


def compare(name, dev, want=WANT_ALL):
    case, ref = case_of(name)
    got = shade(case, dev, want)
    check(case, got, ref, name)
    return case, ref, got


# ---- CPU tests

def test_environment_brdf_against_the_reference_integration():
    from dirt_amd import lighting
    reference, error = R.table_reference_with_error()
    print('table reference: convergence error %.3e' % error)
    assert error <= TABLE_ERROR                      # the recorded figure holds
    tables = {s: lighting.environment_brdf(s) for s in (4, 32)}
    for (s, i, j), ref in zip(R.table_points()[2], reference):
        assert np.abs(tables[s][i, j].double().numpy() - ref).max() <= KERNEL * TABLE_ERROR, (s, i, j, tables[s][i, j], ref)
    for t in tables.values():
        assert t.dtype == torch.float32 and bool((t >= 0).all()) and float(t.sum(-1).max()) <= 1.
    assert torch.equal(lighting.environment_brdf(4), tables[4]) and tables[32].shape == (32, 32, 2)
    # a mirror seen head on reflects everything: A -> 1, B -> 0 as rho -> 0 and nv -> 1
    assert float(tables[32][0, 31, 0]) > 0.99 and float(tables[32][0, 31, 1]) < 1.e-6
    for bad in (1, 2.5, True, '4'):
        with pytest.raises(ValueError, match='size must be an int >= 2'):
            lighting.environment_brdf(bad)
    for bad in ((0, 4), 7, (4,), ('a', 'b')):
        with pytest.raises(ValueError, match='samples must be two positive ints'):
            lighting.environment_brdf(4, samples=bad)


def test_the_restatement_is_image_based_lighting():
    """`terms` of the reference, written from the look-ups, adds up to `lighting.image_based_lighting`, in float64 to rounding"""
    for name in ('pixels_%d' % FLAT, 'env_12_3_5_32', 'scenes_mixed', 'layout_t6', 'tile_edge_and_corner'):
        _, ref = case_of(name)
        assert float((sum(ref['terms']) - ref['pre']).abs().max()) <= 1.e-14, name


def test_the_float32_composition_stays_within_the_committed_figures():
    worst = R.measure_f32(c.measure() for c in (case_of(name)[0] for name in CASES))
    print({k: '%.3e' % v for k, v in worst.items()})
    for k, v in worst.items():
        assert 0 < v <= F32[k], (k, v)


def test_the_cases_hold_what_their_names_say():
    from dirt_amd.texture import directions_to_cube_indices
    for name in CASES:
        case, ref = case_of(name)
        assert case.share < R.MAX_REDRAWN or case.n < 64, (name, case.share)
        assert float(R.kink_distance(ref, case.env, case.kw['clamp'], 0.04).min()) >= R.MARGIN, name
        r = ref['roughness']
        assert bool(((r > 0.04) & (r < 1.)).all()), name
    for k in AXES:
        _, ref = case_of('face_' + k)
        for d in (ref['R'], ref['normals']):
            assert bool((directions_to_cube_indices(d, 8)[0] == FACE[k]).all()), k
    # the tile that is to take the scatter's LDS patch: R and n each on one face, lod inside one pair of levels (the trilinear
    # kernel's condition), and the bounding boxes of the taps fit the patch
    case, ref = case_of('tile_one_face')
    patch = int(re.search(r'constexpr int TEX_PATCH = (\d+);', open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_texture_common.h')).read()).group(1))
    assert set(torch.floor(ref['lam']).long().tolist()) == {1}

    def box(d, n):
        face, index, valid = directions_to_cube_indices(d, n)
        assert bool(valid.all()) and bool((face == 4).all())
        lo, hi = torch.floor(index).amin(0), (torch.floor(index) + 1).clamp(max=n - 1).amax(0)
        return int(((hi - lo + 1)[0] * (hi - lo + 1)[1]).item())

    assert box(ref['R'], case.env.size >> 1) + box(ref['R'], case.env.size >> 2) <= patch and box(ref['normals'], case.env.irradiance_size) <= patch
    _, ref = case_of('tile_edge_and_corner')
    for d in (ref['R'], ref['normals']):
        assert set(directions_to_cube_indices(d, 8)[0].tolist()) == {0, 2, 4}     # the three faces that meet at (1, 1, 1)
    case, ref = case_of('pixels_%d' % FLAT)
    lam = ref['lam']
    assert set(torch.floor(lam).long().tolist()) == {0, 1, 2}                      # every pair of adjacent levels is blended
    m = torch.from_numpy(case.g[:, case.layout['mask']])
    assert bool((m == 0).any()) and bool((m == 1).any()) and bool(((m > 0) & (m < 1)).any())


def _furnace(mu, radiance=0.7, intensity=(0.5, 1., 2.)):
    from dirt_amd import lighting
    rng = np.random.default_rng(5)
    v = 40
    n = torch.from_numpy(rng.standard_normal((v, 3)))
    n = n / n.norm(dim=-1, keepdim=True)
    p = torch.from_numpy(rng.uniform(-1., 1., (v, 3)))
    r = torch.from_numpy(rng.uniform(0., 1.2, v))
    levels = [torch.full((6, 4 >> k, 4 >> k, 3), radiance, dtype=torch.float64) for k in range(3)]
    table = torch.from_numpy(R.brdf_table(16)).double()
    cam = torch.tensor([0.25, -0.5, 4.], dtype=torch.float64)
    out = lighting.image_based_lighting(p, n, torch.ones(v, 3, dtype=torch.float64), r, torch.full((v,), mu, dtype=torch.float64), cam, levels,
                                        levels[1], table, torch.tensor(intensity, dtype=torch.float64))
    N, vv = n, torch.nn.functional.normalize(cam - p, dim=-1)
    nv = (N * vv).sum(-1).clamp(min=0.)
    ab = R._bilinear(table, (r.clamp(0.04, 1.) * 16 - 0.5).clamp(0., 15.), (nv * 16 - 0.5).clamp(0., 15.))
    S = (0.04 * (1. - mu) + mu) * ab[:, :1] + ab[:, 1:]
    return out, S, torch.tensor(intensity, dtype=torch.float64) * radiance


def test_the_white_furnace():
    """a constant environment and a white albedo: intensity L (S + (1 - S)(1 - mu)) per channel; a metal reflects S spec alone"""
    for mu in (0., 0.3, 1.):
        out, S, scale = _furnace(mu)
        assert out.dtype == torch.float64
        assert float((out - scale * (S + (1. - S) * (1. - mu))).abs().max()) <= 1.e-14, mu
        assert bool((out <= scale + 1.e-14).all())          # nothing reflects more than it receives
    out, S, scale = _furnace(1.)
    assert float((out - scale * S).abs().max()) <= 1.e-14


def test_mistakes_show_in_the_reference():
    """each deliberate mistake moves some result by more than the bound the kernel is held to, by a factor recorded above.  The
    pixels are drawn anew with roughness on both sides of its range: inside it, lod from r is lod from rho"""
    rng = np.random.default_rng(99)
    cg, layout = LAYOUTS['c12']
    env = R.Environment(rng, *BASE_ENV)
    g, _, _ = R.random_pixels(rng, 600, cg, layout)
    g[:, layout['material']] = rng.uniform(-0.2, 1.3, 600)
    go = rng.standard_normal((600, 3)).astype(np.float32)
    kw = dict(grad_out=go, clamp=None, camera_position=(0.25, -0.5, 4.), background=(0.2, 0.3, 0.4))
    ref = R.compose(g, env, layout, **kw)
    least = np.inf
    for mistake in R.MISTAKES:
        moved = R.ratios(R.compose(g, env, layout, masses=False, mistake=mistake, **kw), ref)
        most = max(v / (KERNEL * F32[k]) for k, v in moved.items())
        print(mistake, '%.3g' % most)
        least = min(least, most)
    assert least >= SENSITIVITY > 100.


G = torch.zeros(4, 5, 12)
CPU = 'dirt_amd.shading.shade_gbuffer_ibl runs on an MI355X only; there is no CPU fallback'


def test_shade_gbuffer_ibl_refuses_bad_arguments():
    from dirt_amd import shading, texture
    ramp = (0., 0.5, 1.)
    good = texture.CubePyramid(torch.zeros(6, 63), 4, 3, 3, ramp)

    def call(g=G, specular=good, irradiance=torch.zeros(6, 2, 2, 3), brdf=torch.zeros(8, 8, 2), **kw):
        args = dict(colors=4, material=10, normals=7, positions=1, mask=0, camera_position=(0., 0., 4.))
        args.update(kw)
        return shading.shade_gbuffer_ibl(g, specular, irradiance, brdf, **args)

    for kw, text in (
            (dict(g=torch.zeros(5)), 'shade_gbuffer_ibl expects gbuffer [H, W, Cg], [B, H, W, Cg] or [N, Cg], got (5,)'),
            (dict(g=G.to(torch.int32)), 'shade_gbuffer_ibl expects a float32 gbuffer, got torch.int32'),
            (dict(specular=torch.zeros(6, 63)), 'shade_gbuffer_ibl expects specular to be the CubePyramid of prefilter_cube, got Tensor'),
            (dict(specular=texture.CubePyramid(torch.zeros(6, 63), 4, 3, 3)),
             'shade_gbuffer_ibl: specular is a box-filtered pyramid (roughness None): the look-up at lod = roughness (L - 1) needs the levels '
             'prefilter_cube convolves'),
            (dict(specular=texture.CubePyramid(torch.zeros(6, 63), 4, 3, 3, (0., 0.25, 1.))),
             'shade_gbuffer_ibl: specular was filtered at the roughnesses (0.0, 0.25, 1.0), the look-up at lod = roughness (L - 1) needs the '
             'default ramp k / (L - 1) of prefilter_cube'),
            (dict(specular=texture.CubePyramid(torch.zeros(6, 84), 4, 4, 3, ramp)), 'shade_gbuffer_ibl: specular has 4 channels, an environment has 3'),
            (dict(specular=texture.CubePyramid(torch.zeros(6, 60), 4, 3, 3, ramp)),
             'shade_gbuffer_ibl: specular.packed must be [6, 63], the 3 levels of a 4 x 4 x 3 face, got (6, 60)'),
            (dict(specular=texture.CubePyramid(torch.zeros(6, 63), 4, 3, 2, (0., 1.))),
             'shade_gbuffer_ibl: specular.packed must be [6, 60], the 2 levels of a 4 x 4 x 3 face, got (6, 63)'),
            (dict(irradiance=torch.zeros(6, 2, 3, 3)), 'shade_gbuffer_ibl expects irradiance to be a floating-point tensor [6, size, size, 3], got (6, 2, 3, 3)'),
            (dict(irradiance=torch.zeros(6, 2, 2, 4)), 'shade_gbuffer_ibl expects irradiance to be a floating-point tensor [6, size, size, 3], got (6, 2, 2, 4)'),
            (dict(brdf=torch.zeros(1, 1, 2)),
             'shade_gbuffer_ibl expects brdf to be a floating-point tensor [S, S, 2] with 2 <= S <= 128 (lighting.environment_brdf), got (1, 1, 2)'),
            (dict(brdf=torch.zeros(129, 129, 2)),
             'shade_gbuffer_ibl expects brdf to be a floating-point tensor [S, S, 2] with 2 <= S <= 128 (lighting.environment_brdf), got (129, 129, 2)'),
            (dict(brdf=torch.zeros(8, 8, 3)),
             'shade_gbuffer_ibl expects brdf to be a floating-point tensor [S, S, 2] with 2 <= S <= 128 (lighting.environment_brdf), got (8, 8, 3)'),
            (dict(brdf=torch.zeros(8, 8, 2, device='meta')), 'brdf is on meta, the G-buffer on cpu'),
            (dict(irradiance=torch.zeros(6, 2, 2, 3, device='meta')), 'irradiance is on meta, the G-buffer on cpu'),
            (dict(colors=torch.zeros(4, 5, 4)), "colors as a tensor must have shape [4, 5, 3] (the G-buffer's [4, 5, 12] with 3 channels), got [4, 5, 4]"),
            (dict(material=None), 'material must be the index of a G-buffer channel, got None'),
            (dict(material=6), 'material (channel 6) overlaps colors (channel 4)'),
            (dict(positions=None), 'positions must be the index of a G-buffer channel, got None'),
            (dict(mask=12), 'mask at channel 12 does not fit in the 12 channels of the G-buffer'),
            (dict(min_roughness=0.), 'min_roughness must be a number > 0 and <= 1, got 0.0'),
            (dict(dielectric_f0=1.5), 'dielectric_f0 must be a number in [0, 1], got 1.5'),
            (dict(camera_position=None), 'shade_gbuffer_ibl needs camera_position'),
            (dict(clamp=(1., 0.)), 'clamp needs lo <= hi, got (1.0, 0.0)'),
            (dict(intensity=(1., 2.)), 'intensity must be 3 numbers, got 2'),
            (dict(intensity=torch.zeros(2, 3)), 'intensity must have shape [3], got [2, 3]'),
            (dict(background=torch.zeros(4)), 'background must have shape [3], got [4]')):
        with pytest.raises(ValueError) as e:
            call(**kw)
        assert str(e.value) == text, (kw, str(e.value))
    with pytest.raises(RuntimeError) as e:
        call()
    assert str(e.value) == CPU
    with pytest.raises(TypeError):
        shading.shade_gbuffer_ibl(G, good, torch.zeros(6, 2, 2, 3), torch.zeros(8, 8, 2), colors=4, material=10, normals=7, positions=1)


def test_the_functions_are_exported_and_declared():
    import dirt
    import dirt.shading
    import dirt.lighting
    import dirt_amd
    from dirt_amd import _lib, build
    assert dirt.shading.shade_gbuffer_ibl is dirt_amd.shading.shade_gbuffer_ibl
    assert dirt.lighting.image_based_lighting is dirt_amd.lighting.image_based_lighting
    assert dirt.lighting.environment_brdf is dirt_amd.lighting.environment_brdf
    assert 'dirt_shade_ibl.hip' in build.SOURCES and 'dirt_shade_ibl.hip' not in build.PER_SOURCE_FLAGS
    assert 'dirt_texture_cube.h' in build.HEADERS
    header = open(os.path.join(ROOT, 'include', 'dirt_hip.h')).read()
    for symbol in ('dirt_shade_ibl_scratch_bytes', 'dirt_shade_ibl_forward', 'dirt_shade_ibl_backward'):
        assert symbol in _lib.SYMBOLS and re.search(r'\b%s\(' % symbol, header)
    assert '#define DIRT_SHADE_IBL_MAX_TABLE %d\n' % _lib.SHADE_IBL_MAX_TABLE in header and _lib.SHADE_IBL_MAX_TABLE == 128
    assert _lib.ABI_VERSION == 4 and '#define DIRT_ABI_VERSION 4' in header
    source = open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_shade_ibl.hip')).read()
    assert 'atomicAdd' not in source and 'atomic_' not in source and 'powf' not in source and 'asm' not in source
    # one copy of the cube helpers: the header has them, neither unit does
    cube = open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_texture_cube.hip')).read()
    shared = open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_texture_cube.h')).read()
    for helper in ('cube_level_offset(int N', 'struct CubeLook', 'CubeLook cube_look(', 'float cube_index(', 'Taps cube_taps(', 'void cube_direction_gradient('):
        assert helper in shared and helper not in cube and helper not in source, helper
    assert '#include "dirt_texture_cube.h"' in cube and '#include "dirt_texture_cube.h"' in source


def test_one_copy_of_what_the_material_shaders_share():
    """What Cook-Torrance and image-based lighting have in common is declared in dirt_shade_common.h and in neither unit; what
    gave another assembly there (the header says so at each) is written out in both."""
    read = lambda name: open(os.path.join(ROOT, 'dirt_amd', 'csrc', name)).read()   # noqa: E731
    shared, pbr, ibl = read('dirt_shade_common.h'), read('dirt_shade_pbr.hip'), read('dirt_shade_ibl.hip')
    for helper in ('struct MaterialPixel {', 'void material_load(', 'void material_fresnel(', 'int material_source(', 'MATERIAL_ROW = 13',
                   'MATERIAL_ZERO = 12', 'struct MaterialArgs {', 'int material_check_sizes(', 'int material_check_layout(',
                   'int material_check_scalars(', 'int material_check_grads(', 'void material_fill(', 'void material_inputs('):
        assert shared.count(helper) == 1 and helper not in pbr and helper not in ibl, helper
    for unit in (pbr, ibl):
        assert '#include "dirt_shade_common.h"' in unit
        for used in ('material_load(P, prm, pix, px)', 'material_fresnel(P, px)', 'material_source(P, ch)', 'dirt::material_check_sizes(who, a, ',
                     'dirt::material_check_layout(who, a)', 'dirt::material_check_scalars(who, a)', 'dirt::material_fill(P, a, ',
                     'dirt::material_check_grads(who, a, grad_colors, grad_material)'):
            assert used in unit, used
        assert unit.count('dirt::material_inputs(P, a);') == 2 and unit.count('const dirt::MaterialArgs a{') == 2
        # the messages and the assignments the helpers carry stand in no unit
        for text in ('color_stride=%d', 'material_stride=%d', 'param_scenes=%d', 'unknown flags', 'min_roughness=%g', 'dielectric_f0=%g',
                     'grad_colors without colors', 'grad_material without material', 'P.cstride =', 'P.mstride =', 'P.col =', 'P.min_roughness ='):
            assert text not in unit and text.replace('P.', 'p.') in shared, text
        # per kernel: the fill of the channel map and a lane's stores into its row of the tile
        assert 's_src[ch] = (unsigned char)material_source(P, ch);' in unit and 'r[9] = gr; r[10] = gmu; r[11] = gm;' in unit
    assert 's_src[ch] =' not in shared.replace('s_src[ch] = its source function', '') and 'r[9] = gr' not in shared
    assert 'struct PbrPixel : MaterialPixel { float rho2, a2, k, omk, gv; };' in pbr and 'IblPixel' not in ibl and 'MaterialPixel px;' in ibl
    for name in ('PBR_ROW', 'PBR_ZERO', 'IBL_ROW', 'IBL_ZERO', 'shade_pbr_source', 'shade_ibl_source', 'ibl_pixel'):
        assert name not in pbr + ibl + shared, name


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import _lib, build
    build.build_library()
    return _lib.load()


def test_c_entry_points_refuse_bad_arguments_without_a_device(lib):
    from dirt_amd import _lib
    one = ctypes.c_void_p(16)
    E = _lib.E_INVALID_ARGUMENT
    keys = ('scenes', 'rows', 'cols', 'cg', 'cs', 'ms', 'oc', 'omat', 'on', 'op', 'om', 'ps', 'size', 'levels', 'm', 's', 'mr', 'f0', 'lo', 'hi', 'flags')

    def tail(kw):
        d = dict(scenes=1, rows=8, cols=8, cg=12, cs=0, ms=0, oc=4, omat=10, on=7, op=1, om=0, ps=1, size=8, levels=4, m=4, s=16, mr=0.04, f0=0.04,
                 lo=0., hi=1., flags=1)
        d.update(kw)
        return tuple(d[k] for k in keys) + (None,)

    def fwd(g=one, c=None, mt=None, p=one, pyr=one, irr=one, tab=one, out=one, **kw):
        return lib.dirt_shade_ibl_forward(g, c, mt, p, pyr, irr, tab, out, *tail(kw))

    def bwd(g=one, c=None, mt=None, p=one, pyr=one, irr=one, tab=one, go=one, gg=one, gc=None, gm=None, gp=one, gs=one, gi=one, scratch=one,
            nbytes=1 << 20, **kw):
        return lib.dirt_shade_ibl_backward(g, c, mt, p, pyr, irr, tab, go, gg, gc, gm, gp, gs, gi, scratch, nbytes, *tail(kw))

    for who, call in (('dirt_shade_ibl_forward', fwd), ('dirt_shade_ibl_backward', bwd)):
        for kw, text in ((dict(cg=1025), '%s: 1025 G-buffer channels, 1..1024'), (dict(cg=0), '%s: 0 G-buffer channels, 1..1024'),
                         (dict(scenes=-1), '%s: negative sizes (scenes=-1 pixels=64)'), (dict(rows=-5), '%s: bad pixel grid (rows=-5 cols=8)'),
                         (dict(rows=1 << 30, cols=1 << 30), '%s: bad pixel grid (rows=1073741824 cols=1073741824)'),
                         (dict(scenes=65536), '%s: 65536 scenes, at most 65535'),
                         (dict(c=one, cs=2), '%s: color_stride=2, a pixel\'s colour is 3 floats'),
                         (dict(mt=one, ms=1), '%s: material_stride=1, a pixel\'s material is 2 floats'),
                         (dict(ps=2), '%s: param_scenes=2 is neither 1 nor scenes=1'),
                         (dict(flags=3), '%s: unknown flags 0x3'),
                         (dict(oc=9), '%s: material (channel 10) overlaps colors (channel 9)'),
                         (dict(oc=-1), '%s: colors at channel -1 does not fit in 12 channels'),
                         (dict(omat=11), '%s: material at channel 11 does not fit in 12 channels'),
                         (dict(on=10), '%s: normals at channel 10 does not fit in 12 channels'),
                         (dict(op=9), '%s: positions (channel 9) overlaps material (channel 10)'),
                         (dict(om=12), '%s: mask at channel 12 does not fit in 12 channels'),
                         (dict(size=0), '%s: pyramid size 0, 1..32768'),
                         (dict(levels=5), '%s: 5 levels, a 8 x 8 face has 1..4'), (dict(levels=0), '%s: 0 levels, a 8 x 8 face has 1..4'),
                         (dict(size=6, levels=3), '%s: 3 levels, a 6 x 6 face has 1..2'),
                         (dict(m=0), '%s: irradiance size 0, 1..32768'),
                         (dict(s=1), '%s: table size 1, 2..128'), (dict(s=129), '%s: table size 129, 2..128'),
                         (dict(mr=0.), '%s: min_roughness=0 is not in (0, 1]'), (dict(mr=float('nan')), '%s: min_roughness=nan is not in (0, 1]'),
                         (dict(f0=2.), '%s: dielectric_f0=2 is not in [0, 1]'),
                         (dict(lo=1., hi=0.), '%s: clamp bounds lo=1 > hi=0')):
            assert call(**kw) == E, (who, kw)
            assert lib.dirt_last_error().decode() == text % who, (who, kw, lib.dirt_last_error())
    # no pixels: success without a launch (the backward clears the cubes' gradients, so none is asked for here); with tensors
    # off_colors and off_material are not read, and the G-buffer may be six channels
    tensors = dict(c=one, cs=3, mt=one, ms=2, oc=-1, omat=-1, cg=6, on=0, op=3, om=-1)
    assert fwd(rows=0) == 0 and fwd(scenes=0) == 0 and fwd(rows=0, **tensors) == 0 and lib.dirt_last_error() == b''
    assert bwd(rows=0, gs=None, gi=None) == 0 and bwd(scenes=0, gs=None, gi=None, **tensors) == 0 and lib.dirt_last_error() == b''
    assert fwd(out=None) == E and lib.dirt_last_error().decode() == 'dirt_shade_ibl_forward: gbuffer / params / out is NULL'
    assert fwd(g=None) == E and fwd(p=None) == E
    for kw in (dict(pyr=None), dict(irr=None), dict(tab=None)):
        assert fwd(**kw) == E and lib.dirt_last_error().decode() == 'dirt_shade_ibl_forward: pyramid / irradiance / table is NULL'
        assert bwd(**kw) == E and lib.dirt_last_error().decode() == 'dirt_shade_ibl_backward: pyramid / irradiance / table is NULL'
    assert bwd(go=None) == E and lib.dirt_last_error().decode() == 'dirt_shade_ibl_backward: gbuffer / params / grad_out is NULL'
    assert bwd(gc=one) == E
    assert lib.dirt_last_error().decode() == 'dirt_shade_ibl_backward: grad_colors without colors (the channel path\'s is part of grad_gbuffer)'
    assert bwd(gm=one) == E
    assert lib.dirt_last_error().decode() == 'dirt_shade_ibl_backward: grad_material without material (the channel path\'s is part of grad_gbuffer)'
    # a pyramid capped by max_level: any level count from 1 to the face's own is taken
    for levels in (1, 2, 3, 4):
        assert fwd(rows=0, levels=levels) == 0 and bwd(rows=0, gs=None, gi=None, levels=levels) == 0
    assert bwd(gg=None, gp=None, gs=None, gi=None) == 0      # nothing wanted: nothing is launched
    need = lib.dirt_shade_ibl_scratch_bytes(1, 8, 8)
    assert need == 4 * (9 + 10 * 64) and lib.dirt_shade_ibl_scratch_bytes(3, 1, FLAT) == 4 * (9 * 3 * 2 + 10 * 3 * FLAT)
    for bad in ((-1, 8, 8), (65536, 8, 8), (1, -1, 8), (1, 8, -1), (1, 1 << 30, 1 << 30)):
        assert lib.dirt_shade_ibl_scratch_bytes(*bad) == 0
    assert bwd(nbytes=need - 1) == E
    assert lib.dirt_last_error().decode() == 'dirt_shade_ibl_backward: scratch is NULL or smaller than dirt_shade_ibl_scratch_bytes (%d < %d)' % (need - 1, need)
    assert bwd(scratch=None) == E and bwd(scratch=ctypes.c_void_p(18)) == E and b'4-byte aligned' in lib.dirt_last_error()


def test_the_kernels_use_no_scratch_memory():
    from dirt_amd import build
    res = {k: v for k, v in build.kernel_resources().items() if 'shade_ibl_' in k}
    assert len(res) == 5, sorted(res)       # the forward and <PARAMS, GBUF>
    for name, v in res.items():
        assert v['scratch'] == 0 and v['lds'] <= 16384, (name, v)


# ---- GPU tests

@pytest.mark.gpu
@pytest.mark.parametrize('name', [k for k in CASES if k.startswith(('pixels_', 'scenes_', 'image_', 'no_clamp'))])
def test_pixel_counts_and_scenes_against_the_restatement(gpu, name):
    compare(name, gpu)


@pytest.mark.gpu
@pytest.mark.parametrize('name', [k for k in CASES if k.startswith('env_')])
def test_environment_sizes_against_the_restatement(gpu, name):
    compare(name, gpu)


@pytest.mark.gpu
@pytest.mark.parametrize('name', [k for k in CASES if k.startswith('layout_')])
def test_layouts_against_the_restatement(gpu, name):
    compare(name, gpu)


@pytest.mark.gpu
@pytest.mark.parametrize('name', [k for k in CASES if k.startswith(('face_', 'tile_'))])
def test_look_up_placements_against_the_restatement(gpu, name):
    """every face for R and n; a 16 x 16 tile on one face (the scatter sums in its LDS patch) and one across an edge and a
    corner (it adds straight to memory): both cubes' gradients are the reference's, tap by tap"""
    _, ref, got = compare(name, gpu)
    assert bool(got['d_specular'].abs().sum() > 0) and bool(got['d_irradiance'].abs().sum() > 0)


PATTERNS = [dict([(k, True)]) for k in WANT_ALL] + [dict(WANT_ALL), dict(gbuffer=True, specular=True), {}]


@pytest.mark.gpu
@pytest.mark.parametrize('want', PATTERNS, ids=['+'.join(p) or 'none' for p in PATTERNS])
def test_every_pattern_of_wanted_gradients(gpu, want):
    case, ref = case_of('pattern')
    got = shade(case, gpu, want)
    wanted = {'out'} | {'d_' + k for k in want} | ({'d_normals', 'd_positions'} if want.get('gbuffer') else set())
    assert set(got) == wanted, (sorted(got), sorted(wanted))
    check(case, got, ref, 'pattern %s' % sorted(want))


@pytest.mark.gpu
def test_strided_tensors_are_read_in_place(gpu, monkeypatch):
    """`tex[..., :3]` and `tex[..., 3:5]` of a five-channel look-up: the pointers the C ABI receives are the tensor's own at
    stride 5, and every result but the cubes' has the bits of the run on contiguous copies.  Both gradients are dense."""
    from dirt_amd import _stage, _lib
    case, ref = case_of('pattern')
    seen = []
    call = _stage.call
    monkeypatch.setattr(_stage, 'call', lambda f, dev, *args, **kw: (seen.append((f, args)), call(f, dev, *args, **kw))[1])
    lib = _lib.load()
    plain = shade(case, gpu)
    (forward,) = [a for f, a in seen if f is lib.dirt_shade_ibl_forward]
    assert forward[12:14] == (3, 2)
    tex = torch.full((case.n, 5), 1.e30, device=gpu)
    tex[:, :3], tex[:, 3:5] = torch.from_numpy(case.colors).to(gpu), torch.from_numpy(case.material).to(gpu)
    del seen[:]
    got = shade(case, gpu, colors=tex[:, :3], material=tex[:, 3:5])
    (forward,) = [a for f, a in seen if f is lib.dirt_shade_ibl_forward]
    (backward,) = [a for f, a in seen if f is lib.dirt_shade_ibl_backward]
    assert forward[1:3] == (tex.data_ptr(), tex.data_ptr() + 12) and forward[12:14] == (5, 5)
    assert backward[1:3] == forward[1:3] and backward[20:22] == (5, 5)
    assert got['d_colors'].is_contiguous() and got['d_material'].is_contiguous()
    check(case, got, ref, 'slices of a [N, 5] tensor')
    for k in ('out', 'd_gbuffer', 'd_colors', 'd_material'):
        assert torch.equal(got[k], plain[k]), k
    for k in plain['d_params']:
        assert torch.equal(got['d_params'][k], plain['d_params'][k]), k


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['scenes_per_scene', 'tile_edge_and_corner', 'layout_c257'])
def test_two_runs_give_the_same_bits(gpu, name):
    """... for the pixels and every gradient but the two cubes', which the scatter's direct path adds with float atomics: those
    agree with the reference within the tolerance in both runs"""
    case, ref = case_of(name)
    a, b = shade(case, gpu), shade(case, gpu)
    assert set(a) == set(b)
    for k in a:
        if k == 'd_params':
            assert all(torch.equal(a[k][p], b[k][p]) for p in a[k]), k
        elif k not in ('d_specular', 'd_irradiance'):
            assert torch.equal(a[k], b[k]), k
    check(case, a, ref, name + ' first run')
    check(case, b, ref, name + ' second run')


def _abi(lib, dev, case, n, guard=7):
    """forward and backward through the C ABI on the first n pixels of `case` (a flat list), every output and the scratch inside
    `guard` floats of 12345 on both sides -> the outputs, the guards checked and every word inside written"""
    from dirt_amd import _lib
    env = case.env
    g = torch.from_numpy(case.g[:n]).to(dev).contiguous()
    col = torch.from_numpy(case.colors[:n]).to(dev).contiguous() if case.colors is not None else None
    mat = torch.from_numpy(case.material[:n]).to(dev).contiguous() if case.material is not None else None
    block = torch.from_numpy(np.concatenate([case.params[k] for k in R.PARAMS])[None]).to(dev)
    go = torch.from_numpy(case.go[:n]).to(dev).contiguous()
    pyr, irr, tab = (torch.from_numpy(x).to(dev).contiguous() for x in (env.packed(), env.irradiance, env.table))

    def guarded(count):
        t = torch.full((count + 2 * guard,), 12345., device=dev)
        return t, t[guard:guard + count]

    nbytes = lib.dirt_shade_ibl_scratch_bytes(1, 1, n)
    bufs = {k: guarded(c) for k, c in (('out', 3 * n), ('gg', case.cg * n), ('gc', 3 * n), ('gm', 2 * n), ('gp', 9), ('gs', pyr.numel()),
                                       ('gi', irr.numel()), ('scratch', nbytes // 4))}
    lo, hi = case.kw['clamp']
    lay = case.layout
    tail = (1, 1, n, case.cg, 3 if col is not None else 0, 2 if mat is not None else 0, lay.get('colors', -1), lay.get('material', -1), lay['normals'],
            lay['positions'], lay['mask'] if lay.get('mask') is not None else -1, 1, env.size, len(env.levels), env.irradiance_size, env.table_size,
            case.kw['min_roughness'], case.kw['dielectric_f0'], lo, hi, _lib.SHADE_CLAMP, None)
    cp, mp = (t.data_ptr() if t is not None else None for t in (col, mat))
    p = lambda k: bufs[k][1].data_ptr()   # noqa: E731
    torch.cuda.synchronize()
    _lib.check(lib.dirt_shade_ibl_forward(g.data_ptr(), cp, mp, block.data_ptr(), pyr.data_ptr(), irr.data_ptr(), tab.data_ptr(), p('out'), *tail))
    _lib.check(lib.dirt_shade_ibl_backward(g.data_ptr(), cp, mp, block.data_ptr(), pyr.data_ptr(), irr.data_ptr(), tab.data_ptr(), go.data_ptr(), p('gg'),
                                           p('gc') if col is not None else None, p('gm') if mat is not None else None, p('gp'), p('gs'), p('gi'),
                                           p('scratch'), nbytes, *tail))
    torch.cuda.synchronize()
    for k, (full, inner) in bufs.items():
        if (k == 'gc' and col is None) or (k == 'gm' and mat is None):
            assert bool((full == 12345.).all())
            continue
        assert bool((full[:guard] == 12345.).all()) and bool((full[-guard:] == 12345.).all()), k
        assert not bool((inner == 12345.).any()), k
    return {k: v[1] for k, v in bufs.items()}


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 255, 256, 257, FLAT])
@pytest.mark.parametrize('name', ['pixels_%d' % FLAT, 'pattern'])
def test_the_c_abi_writes_inside_its_outputs(gpu, lib, name, n):
    """Guard values around every output and the scratch stay; every element inside is written.  The per-pixel results are the
    wrapper's on the whole frame (held against the restatement above), bit for bit, for the first n pixels: a pixel's values
    do not depend on how many follow it.  At the whole frame the sums are the wrapper's too, the cubes' within the tolerance."""
    case, ref = case_of(name)
    b = _abi(lib, gpu, case, n)
    got = shade(case, gpu)
    assert torch.equal(b['out'].reshape(n, 3), got['out'][:n]) and torch.equal(b['gg'].reshape(n, case.cg), got['d_gbuffer'][:n])
    if case.colors is not None:
        assert torch.equal(b['gc'].reshape(n, 3), got['d_colors'][:n]) and torch.equal(b['gm'].reshape(n, 2), got['d_material'][:n])
    if n == case.n:
        for i, k in enumerate(R.PARAMS):
            assert torch.equal(b['gp'][3 * i:3 * i + 3], got['d_params'][k]), k
        check(case, {'d_specular': b['gs'], 'd_irradiance': b['gi']}, ref, 'the cubes through the C ABI')


KINK_LAYOUT = dict(mask=0, colors=1, normals=4, positions=7, material=10)
KINK_KW = dict(intensity=(0.9, 0.8, 0.7), camera_position=(0.25, -0.5, 4.), background=(0.2, 0.3, 0.4), clamp=None, min_roughness=0.25, dielectric_f0=0.04)


def _pixels(dev, rows):
    """hand-made pixels [m, c[3], n[3], p[3], r, mu] through the fused call and through the float64 and float32 compositions on the same input"""
    g = np.asarray(rows, np.float32)
    case = Case.__new__(Case)
    case.cg, case.layout, case.batch, case.grid, case.n = 12, KINK_LAYOUT, None, None, len(g)
    case.env = R.Environment(np.random.default_rng(31), *BASE_ENV)
    case.kw = {k: KINK_KW[k] for k in ('clamp', 'min_roughness', 'dielectric_f0')}
    case.params = {k: np.asarray(KINK_KW[k], np.float32) for k in R.PARAMS}
    case.g, case.colors, case.material, case.go, case.scene_index = g, None, None, np.ones((len(g), 3), np.float32), None
    got = shade(case, dev)
    args, kw = case.measure()
    refs = [R.compose(*args, dtype=dt, masses=dt == torch.float64, **kw) for dt in (torch.float64, torch.float32)]
    return got, refs[0], refs[1]


def _near(got, r64, r32):
    """|gpu - f32 composition| and |gpu - ref64| within KERNEL x F32 of the float64 masses, non-finite values in the same places"""
    triples = [(kind, got[key], r64[key], r32[key], r64[mass]) for kind, key, mass in R.PAIRS]
    triples += [('d_params', got['d_params'][k], r64['d_params'][k], r32['d_params'][k], r64['mass_params'][k]) for k in got['d_params']]
    for kind, a, ref64, ref32, mass in triples:
        a = a.detach().cpu().double().reshape(ref64.shape)
        for r in (ref64, ref32.double()):
            assert torch.equal(torch.isfinite(a), torch.isfinite(r)), kind
            ok = torch.isfinite(r)
            bound = KERNEL * F32[kind] * mass
            assert bool(((a - r).abs()[ok] <= bound[ok]).all()), (kind, a, r, bound)


N1, P1 = [0.3, -0.2, 0.9], [0.1, 0.2, -0.3]


@pytest.mark.gpu
def test_kink_roughness_outside_its_range(gpu):
    """r below min_roughness and above 1: the clamped value is used and r gets no gradient; at the lower edge itself it does (at
    r = 1 the roughness clamp passes it, but lod sits at its top and the table's row index beyond its last texel: both hold it back)"""
    got, r64, r32 = _pixels(gpu, [[1., .5, .6, .7] + N1 + P1 + [r, 0.5] for r in (0.1, 0.25, 1., 1.5, -1.)])
    _near(got, r64, r32)
    d_r = got['d_material'][:, 0]
    assert not bool(d_r[[0, 3, 4]].any()) and bool(d_r[1] != 0)


@pytest.mark.gpu
def test_kink_a_surface_seen_from_behind(gpu):
    """nv_raw < 0: nv is 0 and passes no gradient, R keeps the unclamped product"""
    got, r64, r32 = _pixels(gpu, [[1., .5, .6, .7] + [-x for x in N1] + P1 + [0.5, 0.5], [0.5, .5, .6, .7, 0.9, 0.1, -0.4] + P1 + [0.7, 0.2]])
    _near(got, r64, r32)
    assert bool((r64['nv_raw'] < 0).all())


@pytest.mark.gpu
def test_kink_metalness_zero_and_one(gpu):
    got, r64, r32 = _pixels(gpu, [[1., .5, .6, .7] + N1 + P1 + [0.5, mu] for mu in (0., 1.)])
    _near(got, r64, r32)
    assert bool(got['d_irradiance'].abs().sum() > 0)       # (the dielectric pixel's)


@pytest.mark.gpu
def test_kink_the_point_at_the_camera(gpu):
    """p = camera: v = 0 with gradient 0, nv_raw = 0, R = 0 is no direction: no specular term, and finite gradients"""
    got, r64, r32 = _pixels(gpu, [[1., .5, .6, .7] + N1 + list(KINK_KW['camera_position']) + [0.5, 0.5]])
    _near(got, r64, r32)
    assert not bool(got['d_specular'].any()) and bool(torch.isfinite(got['d_gbuffer']).all())


@pytest.mark.gpu
def test_kink_a_background_pixel(gpu):
    """a zero normal with m = 0: E is invalid and 0, the pixel is the background, no gradient reaches either cube or the pixel's
    attributes but the mask"""
    got, r64, r32 = _pixels(gpu, [[0., .5, .6, .7, 0., 0., 0.] + P1 + [0.5, 0.5]])
    _near(got, r64, r32)
    assert torch.equal(got['out'].cpu(), torch.tensor([KINK_KW['background']]))
    assert not bool(got['d_specular'].any()) and not bool(got['d_irradiance'].any())
    assert not bool(got['d_gbuffer'][:, 1:].any())


@pytest.mark.gpu
def test_graph_capture_replays_on_changed_inputs(gpu):
    """Forward and backward captured with torch.cuda.graph (the call makes no host synchronisation), replayed once after the
    inputs were overwritten in place: the replay has the eager bits of the new inputs, the cubes' gradients its values."""
    from dirt_amd import shading, texture
    case, _ = case_of('pattern')
    other = Case(seed=6052, n=FLAT, layout='t6')
    eager, ref = shade(other, gpu), other.reference()
    t = lambda x: torch.from_numpy(x).to(gpu)   # noqa: E731
    env = case.env
    g, col, mat, packed, irr = (t(x).requires_grad_(True) for x in (case.g, case.colors, case.material, env.packed(), env.irradiance))
    prm = {k: t(v).requires_grad_(True) for k, v in case.params.items()}
    go, table = t(case.go), t(env.table)
    names = list(prm)
    levels = len(env.levels)

    def step():
        pyramid = texture.CubePyramid(packed, env.size, 3, levels, tuple(k / (levels - 1) for k in range(levels)))
        out = shading.shade_gbuffer_ibl(g, pyramid, irr, table, colors=col, material=mat, normals=case.layout['normals'],
                                        positions=case.layout['positions'], intensity=prm['intensity'], camera_position=prm['camera_position'],
                                        background=prm['background'], clamp=case.kw['clamp'])
        return (out,) + torch.autograd.grad(out, [g, col, mat, packed, irr] + [prm[k] for k in names], go)

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
        for dst, src in [(g, other.g), (col, other.colors), (mat, other.material), (go, other.go), (packed, other.env.packed()),
                         (irr, other.env.irradiance)] + [(prm[k], other.params[k]) for k in names]:
            dst.copy_(t(src))
    for x in captured:
        x.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for x, k in zip(captured[:4], ('out', 'd_gbuffer', 'd_colors', 'd_material')):
        assert torch.equal(x.reshape(eager[k].shape), eager[k]), k
    for x, k in zip(captured[6:], names):
        assert torch.equal(x, eager['d_params'][k]), k
    check(other, {'d_specular': captured[4], 'd_irradiance': captured[5]}, ref, 'the replayed cubes')


def _load(folder, name):
    spec = importlib.util.spec_from_file_location('%s_%s' % (folder, name), os.path.join(ROOT, folder, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_rasterise_deferred_with_the_filters_in_the_shader(gpu):
    """The example's sphere on a 48 x 36 frame through rasterise_deferred, `prefilter_cube` and `convolve_cube(kind='lambert')`
    inside the shader, against the same shader composed of the existing ops on the same GPU (tools/bench_shade_ibl.py::composed:
    the reflection in torch, sample_cube_pyramid, sample_texture_cube, the table look-up and the combine in torch).  The pixels and
    the gradients arriving at the pyramid and at the irradiance cube by the mass rule, masses from the restatement on the rasterised
    G-buffer and the two filtered cubes.  The gradient that reaches the environment by the same rule, every element: the restatement's
    two cube gradients, and F32 x their masses, are carried to the environment's texels by the filters' own backward (the existing
    kernels, linear, with weights >= 0: a texel's mass is the sum of the masses it feeds)."""
    import dirt_amd
    from dirt_amd import shading, texture
    ex = _load('examples', 'fit_material_environment_fused')
    composed = _load('tools', 'bench_shade_ibl').composed
    W, H = 48, 36
    table = R.brdf_table(16)
    brdf = torch.from_numpy(table).to(gpu)
    results = []
    for fused in (False, True):
        scene = ex.Scene(gpu)
        environment = ex.true_environment(ex.SIZE, gpu).requires_grad_(True)
        seen = {}

        def fn(gbuffer, env):
            pyramid, irradiance = ex.filtered(env)
            pyramid.packed.retain_grad(), irradiance.retain_grad()
            seen.update(gbuffer=gbuffer.detach(), pyramid=pyramid, irradiance=irradiance)
            if fused:
                return shading.shade_gbuffer_ibl(gbuffer, pyramid, irradiance, brdf, camera_position=ex.CAMERA, background=ex.BACKGROUND, **ex.LAYOUT)
            return composed(gbuffer, pyramid, irradiance, brdf, camera_position=ex.CAMERA, background=ex.BACKGROUND, **ex.LAYOUT)

        pixels = dirt_amd.rasterise_deferred(torch.zeros([H, W, ex.CHANNELS], device=gpu), scene.clip(W, H), scene.attributes(), scene.faces, fn, [environment])
        (pixels ** 2).mean().backward()
        results.append((pixels.detach(), seen['pyramid'].packed.grad, seen['irradiance'].grad, environment.grad, seen))
    (pa, sa, ia, ea, _), (pb, sb, ib, eb, seen) = results
    assert 0.1 < float((seen['gbuffer'][..., 0] > 0).float().mean()) < 0.9
    pyramid = seen['pyramid']
    env = R.Environment.__new__(R.Environment)
    env.size, env.irradiance_size, env.table_size, env.table = pyramid.size, int(seen['irradiance'].shape[1]), 16, table
    env.levels = [pyramid.level(k).detach().cpu().numpy() for k in range(pyramid.levels)]
    env.irradiance = seen['irradiance'].detach().cpu().numpy()
    go = (2. / pa.numel()) * pa.reshape(-1, 3).cpu().numpy()
    ref = R.compose(seen['gbuffer'].reshape(-1, ex.CHANNELS).cpu().numpy(), env, ex.LAYOUT, camera_position=ex.CAMERA, background=ex.BACKGROUND, grad_out=go)
    for kind, a, b, key in (('pixels', pa, pb, 'out'), ('d_specular', sa, sb, 'd_specular'), ('d_irradiance', ia, ib, 'd_irradiance')):
        r, mass = ref[key], ref[{k: m for _, k, m in R.PAIRS}[key]]
        a, b = a.cpu().double().reshape(mass.shape), b.cpu().double().reshape(mass.shape)
        for x, y, factor in ((b, r, KERNEL), (b, a, KERNEL + 1)):     # against the restatement; against the composed shader, which has its own F32
            assert bool(((x - y).abs() <= factor * F32[kind] * mass).all()), (kind, float(((x - y).abs() / mass.clamp_min(1e-300)).max()), F32[kind])
    # the environment: what arrives at the two cubes goes on through the filters' backward, which is linear with weights >= 0, so
    # the same backward carries the restatement's gradients and its masses (each with its own F32) to the environment's texels
    def through_the_filters(at_pyramid, at_irradiance):
        e = torch.zeros_like(ea).requires_grad_(True)
        pyr, irr = ex.filtered(e)
        t = lambda x, like: x.to(torch.float32).to(gpu).reshape(like.shape)   # noqa: E731
        return torch.autograd.grad([pyr.packed, irr], [e], [t(at_pyramid, pyr.packed), t(at_irradiance, irr)])[0].cpu().double()

    r = through_the_filters(ref['d_specular'], ref['d_irradiance'])
    mass = through_the_filters(F32['d_specular'] * ref['mass_specular'], F32['d_irradiance'] * ref['mass_irradiance'])   # F32 x mass, per texel
    a, b = ea.cpu().double(), eb.cpu().double()
    assert bool(b.abs().max() > 0) and bool((mass >= 0).all())
    for x, y, factor in ((b, r, KERNEL), (b, a, KERNEL + 1)):
        print('deferred: d environment: %.2e of the bound' % float(((x - y).abs() / (factor * mass).clamp_min(1e-300))[mass > 0].max()))
        assert bool(((x - y).abs() <= factor * mass).all())
        assert torch.equal(x[mass == 0], y[mass == 0])


@pytest.mark.gpu
def test_the_example_recovers_material_and_environment(gpu):
    ex = _load('examples', 'fit_material_environment_fused')
    losses, before, after = ex.fit(width=64, height=48, steps=30, device=gpu)
    assert losses[-1] < losses[0] and after < before
