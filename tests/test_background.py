"""`shading.environment_background` (dirt_background.hip) and its torch form `lighting.environment_background`, by the method of
the fused stages: tests/background_reference.py restates the specification of DESIGN.md §7i in float64; the float32 torch
form's worst |f32 - ref64| / mass per kind of result over the cases of `tolerance_cases` is the F32 table below (`python -m
tests.background_reference` prints it), and the kernel gets KERNEL times that, per element against the element's L1 mass.  An
element of zero mass must be exact.  Pixels within OFF_KINKS of a kink -- a face boundary, a texel lattice line of a touched
level, an end of the clamped index, a footprint lambda within 0.05 of an integer, h.w = 0 --, judged by the float64 values
alone, are not compared and carry a zero incoming gradient, so that they add to no sum."""
import ctypes
import functools
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import background_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# python -m tests.background_reference
F32 = {'out': 1.43e-5, 'd_environment': 2.00e-4, 'd_matrix': 8.40e-8, 'd_intensity': 2.64e-6, 'd_mask': 6.86e-6}
KERNEL = 4     # the kernel's allowance over the float32 torch form
TILE = 16      # the side of a backward tile of an image
TEX_PATCH = int(re.search(r'constexpr int TEX_PATCH = (\d+);', open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_texture_common.h')).read()).group(1))

# six rotations of a camera at the centre of the cube; its field of view (right / near = 1.5: 113 degrees) puts the rays of
# one image on three faces, and the six together put every face under at least 8 pixels (test_the_cases_keep_their_classes)
ROTATIONS = [(0.5, 0.6, 0.2), (-0.4, 2.2, 0.3), (0.3, -1.2, -0.5), (1.3, 0.3, 0.2), (-1.2, -0.4, 0.6), (0.2, 3.4, -0.7)]


def camera(rotation, size, translation=(0., 0., 0.), right=0.15, orthographic=False):
    """clip -> world of a camera at `translation` turned by the angle-axis `rotation`, float32 [4, 4]: inverse(view @ projection)"""
    from dirt_amd import matrices
    f64 = lambda x: torch.tensor(x, dtype=torch.float64)   # noqa: E731
    view = matrices.compose(matrices.translation(-f64(translation)), matrices.rodrigues(f64(rotation)))
    projection = (matrices.orthographic_projection if orthographic else matrices.perspective_projection)(f64(0.1), 10., right, size[0] / size[1])
    M = np.ascontiguousarray(torch.linalg.inv(matrices.compose(view, projection)).numpy().astype(np.float32))
    if orthographic:
        M[:, 3] = (0., 0., 0., 1.)      # an affine matrix's inverse is affine: h.w = 1 exactly, whatever the inversion rounded
    return np.ascontiguousarray(M)      # (the inverse comes back column-major, and numpy keeps that through astype and stack)


def masks(kind, size, rng):
    H, W = size
    if kind == 'disc':
        r, c = np.mgrid[0:H, 0:W]
        return (((r - H / 2.) ** 2 + (c - W / 2.) ** 2) < (min(H, W) / 3.) ** 2).astype(np.float32)
    if kind == 'fraction':
        return rng.uniform(0.05, 0.95, size).astype(np.float32)
    if kind == 'mixed':      # covered, background, and the fractions an antialiased edge leaves
        m = rng.uniform(0.05, 0.95, size).astype(np.float32)
        u = rng.uniform(0., 1., size)
        m[u < 0.2], m[u > 0.7] = 1., 0.
        return m
    return {'none': None, 'zero': np.zeros(size, np.float32), 'one': np.ones(size, np.float32)}[kind]


class Case:
    """One call: the environment's levels (float32 values) and how it is passed ('cube': levels[0], of which the others are the
    box pyramid; 'packed': a CubePyramid of the levels), matrices [4, 4] or [B, 4, 4], mask None, [H, W] or [B, H, W], intensity
    [3] or [B, 3], the filter's arguments, and an incoming gradient with zeros on the kinks"""

    def __init__(self, levels, operand, M, size, mask, intensity, kw, seed):
        self.levels, self.operand, self.M, self.size, self.mask, self.kw = levels, operand, np.ascontiguousarray(M, np.float32), size, mask, kw
        self.intensity = np.asarray(intensity, np.float32)
        lead = [x.shape[0] for x, rank in ((self.M, 3), (self.intensity, 2)) if x.ndim == rank] + ([mask.shape[0]] if mask is not None and mask.ndim == 3 else [])
        self.batch = lead[0] if lead else None
        shape = ((self.batch,) if lead else ()) + tuple(size) + (3,)
        go = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
        self.go, self.share = R.off_kinks(self.args[0], dict(self.args[1], grad_out=go))

    @property
    def args(self):
        return (self.levels, self.M, self.size), dict(self.kw, mask=self.mask, intensity=self.intensity, grad_out=getattr(self, 'go', None))

    @functools.cached_property
    def ref(self):
        args, kw = self.args
        return R.compose_batch(*args, **kw)

    @property
    def keep(self):
        return self.ref['valid'] & (self.ref['kink'] >= R.OFF_KINKS)


def make(seed, size, n=12, filter='bilinear', rotation=0, mask='mixed', intensity=(0.7, 1.1, -0.4), operand='cube', max_level=None, levels=None,
         M=None, **kw):
    rng = np.random.default_rng(seed)
    cube = rng.standard_normal((6, n, n, 3)).astype(np.float32)
    if levels is None:
        levels = R.box_levels(cube, max_level) if filter == 'trilinear' else [cube]
    M = camera(ROTATIONS[rotation], size) if M is None else M
    return Case(levels, operand, M, size, masks(mask, size, rng) if isinstance(mask, str) else mask, intensity, dict(kw, filter=filter), seed + 1)


def singular_matrix(size):
    """A camera whose h(0).w is nx: zero on the middle column of an image of odd width (nx = 0 there exactly)"""
    M = camera(ROTATIONS[0], size)
    M[:, 3] = (1., 0., 0.4, 0.)
    return M


def batch_case(seed, matrices, mask, intensity, filter='bilinear', **kw):
    """B = 3 scenes of 17 x 19 pixels; `matrices`, `mask`, `intensity`: 'shared' or 'scene'"""
    size, rng = (17, 19), np.random.default_rng(seed)
    M = np.stack([camera(ROTATIONS[b], size) for b in range(3)]) if matrices == 'scene' else camera(ROTATIONS[3], size)
    m = np.stack([masks(k, size, rng) for k in ('mixed', 'disc', 'fraction')]) if mask == 'scene' else (masks('mixed', size, rng) if mask == 'shared' else None)
    I = rng.uniform(-1., 1., (3, 3)) if intensity == 'scene' else (0.7, 1.1, -0.4)
    return make(seed, size, filter=filter, M=M, mask=m, intensity=I, **kw)


# every legal mix of shared and per-scene operands with B = 3 (at least one per scene, or there is no batch)
BATCH_MIXES = [(a, b, c) for a in ('scene', 'shared') for b in ('scene', 'shared', 'none') for c in ('scene', 'shared') if 'scene' in (a, b, c)]


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith('rotation-'):          # 17 x 19: partial tiles on both edges
        k = int(name.split('-')[1])
        return make(10 + k, (17, 19), rotation=k, filter=('bilinear', 'nearest', 'trilinear')[k % 3], **(dict(lod=0.7) if k % 3 == 2 else {}))
    if name == 'tile':
        return make(20, (16, 16))
    if name == 'pixel':
        return make(21, (1, 1), mask='none')
    if name == 'tall':
        return make(22, (33, 16), rotation=2)
    if name == 'translated':
        return make(23, (17, 19), M=camera(ROTATIONS[1], (17, 19), translation=(0.3, -0.2, 0.1)))
    if name == 'orthographic':                # every ray has one direction, the footprint is 0: lambda clamps to 0
        return make(24, (17, 19), filter='trilinear', M=camera(ROTATIONS[0], (17, 19), orthographic=True), lod=None)
    if name == 'orthographic-bilinear':
        return make(24, (17, 19), M=camera(ROTATIONS[0], (17, 19), orthographic=True))
    if name == 'singular':
        return make(25, (17, 19), M=singular_matrix((17, 19)))
    if name.startswith('size-'):              # N = 1, 4, 5, 12; trilinear where the size has levels
        n = int(name.split('-')[1])
        return make(30 + n, (17, 19), n=n, rotation=n % 6, **(dict(filter='trilinear', lod=0.6) if n % 2 == 0 else {}))
    if name == 'nearest':
        return make(40, (16, 16), n=5, filter='nearest', rotation=4)
    if name == 'lod-0':                       # equals bilinear to the bit
        return make(41, (17, 19), filter='trilinear', lod=0.)
    if name == 'lod-0-bilinear':
        return make(41, (17, 19))
    if name == 'lod-0.7':
        return make(42, (17, 19), filter='trilinear', lod=0.7, rotation=1)
    if name == 'lod-top':
        return make(43, (17, 19), filter='trilinear', lod=5., rotation=2)
    if name == 'lod-bias':
        return make(44, (17, 19), filter='trilinear', lod=0.4, lod_bias=0.9, rotation=3)
    if name == 'max-level':
        return make(45, (17, 19), filter='trilinear', lod=0.7, max_level=1, rotation=4)
    if name == 'footprint':                   # lambda from below 0 to above 1: both level pairs of a 12 x 12 cube
        return make(46, (33, 16), filter='trilinear', lod=None, lod_bias=0.9, rotation=5)
    if name == 'pyramid':                     # a CubePyramid of the box levels: the gradient goes to `packed`
        return make(47, (33, 16), filter='trilinear', lod=None, lod_bias=0.9, operand='packed', rotation=1)
    if name.startswith('mask-'):
        return make(50, (17, 19), mask=name.split('-')[1], rotation=1)
    if name.startswith('batch:'):
        return batch_case(60 + BATCH_MIXES.index(tuple(name.split(':')[1:])), *name.split(':')[1:])
    if name == 'batch-footprint':
        return batch_case(80, 'scene', 'scene', 'shared', filter='trilinear', lod=None, lod_bias=0.9)
    if name == 'one-face':                    # a 16 x 16 tile that sees the middle of one face: its taps fit the LDS patch
        return make(90, (16, 16), M=camera((0., 0., 0.), (16, 16), right=0.03), mask='none')
    raise KeyError(name)


SINGLE_CASES = ['rotation-%d' % k for k in range(6)] + ['tile', 'pixel', 'tall', 'translated', 'orthographic', 'singular', 'size-1', 'size-4', 'size-5',
                                                         'size-12', 'nearest', 'lod-0', 'lod-0.7', 'lod-top', 'lod-bias', 'max-level', 'footprint', 'pyramid',
                                                         'mask-none', 'mask-zero', 'mask-one', 'mask-disc', 'mask-fraction', 'one-face']
BATCH_CASES = ['batch:' + ':'.join(mix) for mix in BATCH_MIXES] + ['batch-footprint']


def tolerance_cases():
    return [case(name).args + (case(name).operand,) for name in SINGLE_CASES + BATCH_CASES]


# ---- without a GPU

def test_the_cases_keep_their_classes():
    """No case takes out more than a tenth of its pixels, and every class a case is there for keeps at least 8 of them"""
    for name in SINGLE_CASES + BATCH_CASES:
        assert case(name).share <= 0.10, (name, case(name).share)

    def kept(name, what):
        c = case(name)
        return c.ref[what][c.keep]

    faces = sum(np.bincount(kept('rotation-%d' % k, 'face'), minlength=6) for k in range(6))
    assert (faces >= 8).all(), faces
    for k in range(6):
        assert (np.bincount(kept('rotation-%d' % k, 'face'), minlength=6) >= 8).sum() >= 3, k      # the rays of one image reach three faces
    assert kept('tile', 'clamped').sum() >= 8 and kept('footprint', 'clamped').sum() >= 8
    for name, pairs in (('footprint', 2), ('batch-footprint', 2), ('pyramid', 2)):
        c = case(name)
        lower, two = kept(name, 'level'), kept(name, 'two')
        assert [int((two & (lower == l)).sum()) >= 8 for l in range(pairs)] == [True] * pairs, name
        assert (c.ref['lam'][c.keep] < 0).sum() >= 8                                                # ... and the clamp at level 0
    assert (kept('lod-top', 'level') == 2).all() and not kept('lod-top', 'two').any()
    assert (kept('lod-0.7', 'level') == 0).all() and kept('lod-0.7', 'two').all()
    assert (kept('lod-bias', 'level') == 1).all() and kept('lod-bias', 'two').all() and len(case('max-level').levels) == 2
    assert (kept('orthographic', 'lam') == -np.inf).all()
    dead = ~case('singular').ref['valid']
    assert dead[:, 9].all() and (~dead).sum(0)[[8, 10]].min() >= 8      # h.w = nx: the middle column, and only that one
    one = case('one-face')
    box = [b[one.keep] for b in one.ref['box0']]
    assert len(np.unique(kept('one-face', 'face'))) == 1 and (box[1].max() - box[0].min() + 1) * (box[3].max() - box[2].min() + 1) <= TEX_PATCH
    assert len(np.unique(kept('tile', 'face'))) == 3                                                  # a tile that straddles face edges


@pytest.mark.parametrize('name', SINGLE_CASES + BATCH_CASES)
def test_the_float32_torch_form_against_the_restatement(name):
    """Per element, relative to the element's mass: within the F32 table, whose figures are this test's own worst ones"""
    c = case(name)
    args, kw = c.args
    got = R.torch_form(*args, operand=c.operand, **kw)
    worst = R.ratios(got, c.ref, c.operand)
    print(name, {k: '%.2e' % v for k, v in worst.items()})
    for kind, x in worst.items():
        assert x <= F32[kind], (kind, x)
    assert R.exact_where_massless(got, c.ref, c.operand)


@pytest.mark.parametrize('filter', ['nearest', 'bilinear'])
def test_the_torch_form_against_the_composition(filter):
    """`unproject_pixels_to_rays` at the pixel centres -> `directions_to_cube_indices` -> `sample_cube` -> (1 - m) intensity E, in
    float32 like the form: values and autograd gradients, each element within KERNEL F32 of its mass (the two differ in the order
    of the matrix product's terms alone; the bound is the float32 form's own measured error against the restatement)"""
    from dirt_amd import lighting, projection, texture
    c = make(100, (17, 19), n=12, filter=filter, rotation=2)
    H, W = c.size
    leaves = lambda: [torch.tensor(x, requires_grad=True) for x in (c.levels[0], c.M, c.intensity, c.mask)]   # noqa: E731
    cube, M, I, m = leaves()
    form = lighting.environment_background(cube, M, c.size, mask=m, intensity=I, filter=filter)
    form.backward(torch.from_numpy(c.go))
    cube2, M2, I2, m2 = leaves()
    cols, rows = torch.meshgrid(torch.arange(W) + 0.5, torch.arange(H) + 0.5, indexing='xy')
    directions = projection.unproject_pixels_to_rays(torch.stack([cols, rows], -1), M2, (W, H))[1]
    composed = (1. - m2)[..., None] * I2 * texture.sample_cube(cube2, *texture.directions_to_cube_indices(directions, 12), filter)
    composed.backward(torch.from_numpy(c.go))
    ref = c.ref
    names = ('d_environment', 'd_matrix', 'd_intensity', 'd_mask')
    grads = lambda leaves: {k: x.grad if x.grad is not None else torch.zeros_like(x) for k, x in zip(names, leaves)}   # noqa: E731
    a, b = dict(grads((cube, M, I, m)), out=form.detach()), dict(grads((cube2, M2, I2, m2)), out=composed.detach())
    masses = {'out': ref['mass_out'], 'd_environment': ref['mass_d_levels'][0], 'd_matrix': ref['mass_d_matrix'], 'd_intensity': ref['mass_d_intensity'],
              'd_mask': ref['mass_d_mask']}
    for kind, mass in masses.items():
        x, y = a[kind].numpy().astype(np.float64), b[kind].numpy().astype(np.float64)
        if kind in ('out', 'd_mask'):
            x, y, mass = x[c.keep], y[c.keep], mass[c.keep]
        worst = R.worst_ratio(x, y, mass)
        print(filter, kind, '%.2e' % worst)
        assert worst <= KERNEL * F32[kind], (kind, worst)


def test_the_footprint_against_a_finite_difference_of_the_rays():
    """The restatement's analytic footprint is the larger of the two distances, in texels of level 0, between the look-ups of the
    rays one pixel apart along x and along y -- taken as a central difference of its own float64 rays 1e-4 of a pixel apart,
    relative 1e-6, on pixels that keep clear of face edges (both displaced rays on the pixel's own face)"""
    c = case('footprint')
    (H, W), n = c.size, 12
    M = c.M.astype(np.float64)
    ref = R.compose(c.levels, c.M, c.size, filter='trilinear', lod=None)
    rho = 2. ** ref['lam']

    def face_coordinates(nx, ny):
        ends = [np.stack([nx, ny, np.full_like(nx, z), np.ones_like(nx)], -1) @ M for z in (0., -1.)]
        d = ends[0][..., :3] / ends[0][..., 3:] - ends[1][..., :3] / ends[1][..., 3:]
        ad = np.abs(d)
        major = np.where((ad[..., 0] >= ad[..., 1]) & (ad[..., 0] >= ad[..., 2]), 0, np.where(ad[..., 1] >= ad[..., 2], 1, 2))
        face = 2 * major + (np.take_along_axis(d, major[..., None], -1)[..., 0] <= 0)
        a = (d * R.MA[face]).sum(-1)
        return face, np.stack([(d * R.SC[face]).sum(-1) / a, (d * R.TC[face]).sum(-1) / a], -1)

    nx, ny = np.meshgrid(2. * (np.arange(W) + 0.5) / W - 1., 1. - 2. * (np.arange(H) + 0.5) / H)
    step = 1.e-4
    lengths, clear = [], ref['valid'].copy()
    for dx, dy in ((2. / W, 0.), (0., 2. / H)):
        (fa, a), (fb, b) = face_coordinates(nx + step * dx, ny + step * dy), face_coordinates(nx - step * dx, ny - step * dy)
        clear &= (fa == ref['face']) & (fb == ref['face'])
        lengths.append(np.linalg.norm(a - b, axis=-1) / (2. * step))
    fd = n / 2. * np.maximum(*lengths)
    assert clear.sum() >= 0.9 * H * W
    assert (np.abs(fd - rho)[clear] <= 1.e-6 * rho[clear]).all(), (np.abs(fd - rho) / rho)[clear].max()


G = torch.zeros(4, 5, 7)
CUBE = torch.zeros(6, 4, 4, 3)
EYE = torch.eye(4)


def pyramid(floats=63, size=4, channels=3, levels=3):
    from dirt_amd.texture import CubePyramid
    return CubePyramid(torch.zeros(6, floats), size, channels, levels)


REFUSALS = [
    (dict(size=0), 'size must be a positive int or (height, width), got 0'),
    (dict(size=(4, 5, 6)), 'size must be a positive int or (height, width), got (4, 5, 6)'),
    (dict(size=(4, 2.5)), 'size must be a positive int or (height, width), got (4, 2.5)'),
    (dict(filter='cubic'), "environment_background: filter must be 'nearest', 'bilinear' or 'trilinear', got 'cubic'"),
    (dict(lod=1.), "lod, lod_bias and max_level apply to filter='trilinear' only (got filter='bilinear')"),
    (dict(filter='nearest', lod_bias=0.5), "lod, lod_bias and max_level apply to filter='trilinear' only (got filter='nearest')"),
    (dict(max_level=1), "lod, lod_bias and max_level apply to filter='trilinear' only (got filter='bilinear')"),
    (dict(filter='trilinear', max_level=-1), 'max_level must be a non-negative int or None, got -1'),
    (dict(filter='trilinear', lod=torch.zeros(4, 5)), 'lod must be a finite number or None (the footprint of the pixel), got %r' % (torch.zeros(4, 5),)),
    (dict(filter='trilinear', lod=float('nan')), 'lod must be a finite number or None (the footprint of the pixel), got nan'),
    (dict(filter='trilinear', lod_bias=float('inf')), 'lod_bias must be a finite number, got inf'),
    (dict(environment=pyramid()), "environment_background: a CubePyramid is looked up with filter='trilinear', got filter='bilinear'"),
    (dict(environment=pyramid(), filter='trilinear', max_level=1),
     'environment_background: max_level applies to a cube, whose pyramid the call builds; a CubePyramid has its 3 levels'),
    (dict(environment=pyramid(channels=4), filter='trilinear'), 'environment_background: environment has 4 channels, an environment has 3'),
    (dict(environment=pyramid(floats=62), filter='trilinear'),
     'environment_background: environment.packed must be [6, 63], the 3 levels of a 4 x 4 x 3 face, got (6, 62)'),
    (dict(environment=torch.zeros(6, 4, 5, 3)), 'environment_background expects environment to be a cube [6, size, size, 3] or a CubePyramid, got (6, 4, 5, 3)'),
    (dict(environment=[1, 2]), 'environment_background expects environment to be a cube [6, size, size, 3] or a CubePyramid, got list'),
    (dict(environment=torch.zeros(6, 4, 4, 4)), 'environment_background: environment has 4 channels, an environment has 3'),
    (dict(environment=CUBE.double()), 'environment must be float32, got torch.float64'),
    (dict(clip_to_world=torch.zeros(3, 4)), 'clip_to_world must have shape [4, 4] or [B, 4, 4], got (3, 4)'),
    (dict(clip_to_world=EYE.double()), 'clip_to_world must be float32, got torch.float64'),
    (dict(clip_to_world=EYE.to('meta')), 'clip_to_world is on meta, the environment on cpu'),
    (dict(mask=torch.zeros(5, 4)), 'mask must have shape [4, 5] or [B, 4, 5], got (5, 4)'),
    (dict(mask=G[..., 0].to('meta')), 'mask is on meta, the environment on cpu'),
    (dict(mask=torch.zeros(4, 5, dtype=torch.bool)), 'mask must be float32, got torch.bool'),
    (dict(intensity=(1., 2.)), 'intensity must be 3 numbers, got 2'),
    (dict(intensity='abc'), "intensity must be 3 numbers or a tensor, got 'abc'"),
    (dict(intensity=torch.zeros(2, 2)), 'intensity must have shape [3] or [B, 3], got (2, 2)'),
    (dict(clip_to_world=torch.zeros(2, 4, 4), mask=torch.zeros(3, 4, 5)), 'environment_background: 2 scenes of clip_to_world, 3 of mask'),
    (dict(mask=torch.zeros(3, 4, 5), intensity=torch.zeros(2, 3)), 'environment_background: 3 scenes of mask, 2 of intensity'),
]


@pytest.mark.parametrize('change, text', REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_python_refusals_in_full(change, text):
    """Every refusal of `_check_background_arguments` with its full text, before any device work: on a machine without a GPU"""
    from dirt_amd import shading
    kw = dict(dict(environment=CUBE, clip_to_world=EYE, size=(4, 5)), **change)
    environment, clip_to_world, size = kw.pop('environment'), kw.pop('clip_to_world'), kw.pop('size')
    with pytest.raises(ValueError) as e:
        shading.environment_background(environment, clip_to_world, size, **kw)
    assert str(e.value) == text


def test_what_passes_the_checks_needs_the_gpu():
    from dirt_amd import shading
    for environment, kw in ((CUBE, {}), (CUBE, dict(filter='trilinear', max_level=1, lod_bias=0.5)), (pyramid(), dict(filter='trilinear', lod=1))):
        with pytest.raises(RuntimeError) as e:
            shading.environment_background(environment, torch.zeros(2, 4, 4), 4, mask=torch.zeros(7, 4, 4)[0], intensity=torch.zeros(2, 3), **kw)
        assert str(e.value) == 'dirt_amd.shading.environment_background runs on an MI355X only; there is no CPU fallback'


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import _lib
    return _lib.load()


FWD = dict(environment=None, matrices=None, intensity=None, mask=None, out=None, scenes=2, rows=3, cols=4, size=12, levels=1, matrix_scenes=1,
           intensity_scenes=2, mask_scenes=1, mask_stride=1, filter=1, lod=0., lod_bias=0., flags=0, stream=None)
ONE = ctypes.c_void_p(16)      # a pointer that is not NULL and is never dereferenced: every call it is given to is refused first
C_REFUSALS = [
    (dict(scenes=-1), '%s: -1 scenes, 0..65535'),
    (dict(scenes=65536), '%s: 65536 scenes, 0..65535'),
    (dict(rows=-1), '%s: bad pixel grid (rows=-1 cols=4), at most 2^31 - 1 each way and 2^40 pixels'),
    (dict(rows=1 << 30, cols=1 << 30), '%s: bad pixel grid (rows=1073741824 cols=1073741824), at most 2^31 - 1 each way and 2^40 pixels'),
    (dict(cols=1 << 31), '%s: bad pixel grid (rows=3 cols=2147483648), at most 2^31 - 1 each way and 2^40 pixels'),
    (dict(filter=3), '%s: filter=3 is none of DIRT_BACKGROUND_NEAREST, _BILINEAR, _TRILINEAR'),
    (dict(flags=2), '%s: unknown flags 0x2'),
    (dict(flags=1), '%s: DIRT_BACKGROUND_FOOTPRINT applies to DIRT_BACKGROUND_TRILINEAR only (filter=1)'),
    (dict(size=0), '%s: environment size 0, 1..32768'),
    (dict(size=32769), '%s: environment size 32769, 1..32768'),
    (dict(filter=2, levels=4), '%s: 4 levels, a 12 x 12 face has 1..3'),
    (dict(levels=0), '%s: 0 levels, a 12 x 12 face has 1..3'),
    (dict(levels=2), '%s: 2 levels, a look-up that is not trilinear reads a cube of one level'),
    (dict(matrix_scenes=3), '%s: matrix_scenes=3 is neither 1 nor scenes=2'),
    (dict(intensity_scenes=0), '%s: intensity_scenes=0 is neither 1 nor scenes=2'),
    (dict(mask=ONE, mask_scenes=3), '%s: mask_scenes=3 is neither 1 nor scenes=2'),
    (dict(mask=ONE, mask_stride=0), '%s: mask_stride=0, a pixel\'s mask is 1 float'),
    (dict(filter=2, lod=float('nan')), '%s: lod=nan, lod_bias=0: not finite'),
    (dict(filter=2, lod_bias=float('inf')), '%s: lod=0, lod_bias=inf: not finite'),
]


def test_c_refusals_come_before_any_device_work(lib):
    """Every refusal returns DIRT_E_INVALID_ARGUMENT with its sentence in dirt_last_error() -- on a machine without a GPU, with
    NULL pointers: nothing was dereferenced and nothing was launched.  The backward shares the checks and adds its own."""
    from dirt_amd import _lib
    bwd = dict(environment=None, matrices=None, intensity=None, mask=None, grad_out=None, grad_environment=None, grad_matrices=None,
               grad_intensity=None, grad_mask=None, scratch=None, scratch_bytes=0, **{k: FWD[k] for k in list(FWD)[5:]})
    for change, text in C_REFUSALS:
        for name, base in (('dirt_background_forward', FWD), ('dirt_background_backward', bwd)):
            assert getattr(lib, name)(*dict(base, **change).values()) == _lib.E_INVALID_ARGUMENT, (name, change)
            assert _lib.last_error() == text % name, (_lib.last_error(), text % name)
    who = 'dirt_background_forward'
    assert lib.dirt_background_forward(*FWD.values()) == _lib.E_INVALID_ARGUMENT
    assert _lib.last_error() == '%s: environment / matrices / intensity / out is NULL' % who
    assert lib.dirt_background_forward(*dict(FWD, rows=0).values()) == 0 and _lib.last_error() == ''
    assert lib.dirt_background_forward(*dict(FWD, scenes=0, intensity_scenes=1).values()) == 0 and _lib.last_error() == ''
    who = 'dirt_background_backward'
    given = dict(environment=ONE, matrices=ONE, intensity=ONE, grad_out=ONE)
    need = lib.dirt_background_scratch_bytes(2, 3, 4)
    assert need == 4 * (2 * 1 * 19 + 2 * 12 * 7)      # a row of 16 + 3 sums per tile, 7 floats per pixel
    for change, text in [(dict(grad_mask=ONE), '%s: grad_mask without mask' % who),
                         (dict(grad_matrices=ONE), '%s: environment / matrices / intensity / grad_out is NULL' % who),
                         (dict(given, grad_matrices=ONE), '%s: scratch is NULL or smaller than dirt_background_scratch_bytes (0 < %d)' % (who, need)),
                         (dict(given, grad_environment=ONE, scratch=ONE, scratch_bytes=need - 4),
                          '%s: scratch is NULL or smaller than dirt_background_scratch_bytes (%d < %d)' % (who, need - 4, need)),
                         (dict(given, grad_intensity=ONE, scratch=ctypes.c_void_p(18), scratch_bytes=need), '%s: scratch is not 4-byte aligned' % who)]:
        assert lib.dirt_background_backward(*dict(bwd, **change).values()) == _lib.E_INVALID_ARGUMENT, change
        assert _lib.last_error() == text, (_lib.last_error(), text)
    assert lib.dirt_background_backward(*bwd.values()) == 0 and _lib.last_error() == ''      # no gradient wanted: success, nothing is launched
    assert lib.dirt_background_scratch_bytes(-1, 3, 4) == 0 and lib.dirt_background_scratch_bytes(1, 1 << 31, 4) == 0
    assert lib.dirt_background_scratch_bytes(1, 0, 4) == 0 and lib.dirt_background_scratch_bytes(3, 17, 19) == 4 * (3 * 4 * 19 + 3 * 323 * 7)


def test_names_header_and_build():
    """The function under both package names, the header's declarations, the unit in the build without flags of its own"""
    import dirt
    import dirt.shading
    import dirt_amd
    from dirt_amd import _lib, build, lighting, shading
    assert dirt.shading.environment_background is dirt_amd.shading.environment_background is shading.environment_background
    assert dirt.lighting.environment_background is lighting.environment_background
    assert 'dirt_background.hip' in build.SOURCES and 'dirt_background.hip' not in build.PER_SOURCE_FLAGS
    header = open(os.path.join(ROOT, 'include', 'dirt_hip.h')).read()
    for name in ('dirt_background_scratch_bytes', 'dirt_background_forward', 'dirt_background_backward'):
        assert re.search(r'\b%s\(' % name, header) and name in _lib.SYMBOLS
    assert '#define DIRT_ABI_VERSION 4' in header and _lib.ABI_VERSION == 4
    for name, value in (('NEAREST', 0), ('BILINEAR', 1), ('TRILINEAR', 2)):
        assert re.search(r'#define DIRT_BACKGROUND_%s %d\b' % (name, value), header) and _lib.BACKGROUND_FILTERS[name.lower()] == value
    assert re.search(r'#define DIRT_BACKGROUND_FOOTPRINT 1u', header) and _lib.BACKGROUND_FOOTPRINT == 1


# ---- on the GPU: the kernels against the restatement

def _dev(gpu, x):
    return torch.as_tensor(np.ascontiguousarray(x), device=gpu)      # (row-major in memory: the C ABI is handed data pointers)


def run_kernel(c, gpu, want=(True, True, True, True), mask=None, environment=None):
    """`shading.environment_background` on the case -> the keys of `R.torch_form` (a gradient that is not wanted: None).
    `mask`: a tensor to pass in place of the case's (a strided view of the same values); `environment`: likewise"""
    from dirt_amd import shading
    from dirt_amd.texture import CubePyramid
    leaf = _dev(gpu, c.levels[0] if c.operand == 'cube' else R.pack(c.levels)).requires_grad_(want[0]) if environment is None else environment
    env = leaf if c.operand == 'cube' else CubePyramid(leaf, c.levels[0].shape[1], 3, len(c.levels))
    M, I = _dev(gpu, c.M).requires_grad_(want[1]), _dev(gpu, c.intensity).requires_grad_(want[2])
    m = mask if mask is not None else (None if c.mask is None else _dev(gpu, c.mask).requires_grad_(want[3]))
    kw = {k: v for k, v in c.kw.items() if k != 'filter'}
    if c.kw['filter'] == 'trilinear' and c.operand == 'cube':
        kw['max_level'] = len(c.levels) - 1
    out = shading.environment_background(env, M, c.size, mask=m, intensity=I, filter=c.kw['filter'], **kw)
    res = {'out': out.detach().cpu().numpy()}
    leaves = [(k, x) for k, x, on in (('d_environment', leaf, want[0]), ('d_matrix', M, want[1]), ('d_intensity', I, want[2]), ('d_mask', m, want[3]))
              if on and x is not None and x.requires_grad]
    if leaves:
        grads = torch.autograd.grad(out, [x for _, x in leaves], _dev(gpu, c.go))
        res.update({k: g.cpu().numpy() for (k, _), g in zip(leaves, grads)})
    return res


def _check(got, c):
    worst = R.ratios(got, c.ref, c.operand)
    print({k: '%.2e' % v for k, v in worst.items()})
    for kind, x in worst.items():
        assert x == x and x <= KERNEL * F32[kind], (kind, x, KERNEL * F32[kind])
    assert R.exact_where_massless(got, c.ref, c.operand)
    dead = ~c.ref['valid']
    assert not got['out'][dead].any()      # no look-up: exactly 0
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('name', SINGLE_CASES + BATCH_CASES)
def test_kernels_against_the_restatement(gpu, name):
    c = case(name)
    got = run_kernel(c, gpu)
    assert got['out'].shape == (((c.batch,) if c.batch else ()) + tuple(c.size) + (3,))
    _check(got, c)
    if name == 'mask-one':
        assert not got['out'].any() and not got['d_environment'].any() and not got['d_matrix'].any() and not got['d_intensity'].any()
    if name == 'singular':
        assert all(np.isfinite(got[k]).all() for k in got)


@pytest.mark.gpu
@pytest.mark.parametrize('name, twin', [('lod-0', 'lod-0-bilinear'), ('orthographic', 'orthographic-bilinear')])
def test_level_zero_is_bilinear_bit_for_bit(gpu, name, twin):
    """lod = 0, and a footprint of 0 (every ray of an orthographic camera has one direction: lambda = -inf clamps to 0)"""
    a, b = run_kernel(case(name), gpu), run_kernel(case(twin), gpu)
    for k in ('out', 'd_matrix', 'd_intensity', 'd_mask'):
        assert np.array_equal(a[k], b[k]), k
    np.testing.assert_allclose(a['d_environment'], b['d_environment'], rtol=0, atol=1e-5)      # (float atomics: not the same bits)


@pytest.mark.gpu
def test_a_prefiltered_pyramid_serves_the_background(gpu):
    """The pyramid `shade_gbuffer_ibl` holds -- `prefilter_cube`'s, whose levels are no box means -- and `cube_pyramid`'s, made on
    the GPU and read back as the restatement's levels; the gradient arrives at the cube through `packed`"""
    from dirt_amd import shading, texture
    base = case('pyramid')
    cube = _dev(gpu, base.levels[0]).requires_grad_(True)
    for build in (texture.prefilter_cube, texture.cube_pyramid):
        pyr = build(cube)
        levels = [pyr.level(k).detach().cpu().numpy() for k in range(pyr.levels)]
        c = Case(levels, 'packed', base.M, base.size, base.mask, base.intensity, base.kw, 471)
        assert c.share <= 0.10
        packed = pyr.packed.detach().requires_grad_(True)
        _check(run_kernel(c, gpu, environment=packed), c)
        out = shading.environment_background(pyr, _dev(gpu, c.M), c.size, mask=_dev(gpu, c.mask), intensity=tuple(c.intensity), filter='trilinear', lod_bias=0.9)
        grad, = torch.autograd.grad(out, cube, _dev(gpu, c.go))
        assert grad.shape == cube.shape and grad.abs().sum() > 0


@pytest.mark.gpu
def test_a_mask_that_is_a_slice_of_the_gbuffer_is_read_in_place(gpu):
    """mask = gbuffer[..., 3] of a [H, W, 7] G-buffer: the kernel is handed the slice's own address and stride, and torch carries
    the dense gradient back through the slice"""
    from dirt_amd import texture
    c = case('rotation-0')
    g = torch.randn(17, 19, 7, device=gpu)
    g[..., 3] = _dev(gpu, c.mask)
    g.requires_grad_(True)
    view = g[..., 3]
    src, stride = texture._scalars_in_place(view)
    assert src.data_ptr() == g.data_ptr() + 12 and stride == 7
    got = run_kernel(c, gpu, mask=view)
    grad, = torch.autograd.grad(run_kernel_output(c, gpu, view), g, _dev(gpu, c.go))
    _check(dict(got, d_mask=grad[..., 3].cpu().numpy()), c)
    assert not grad[..., :3].any() and not grad[..., 4:].any()
    batch = case('batch:shared:scene:shared')
    gb = torch.randn(3, 17, 19, 7, device=gpu)
    gb[..., 0] = _dev(gpu, batch.mask)
    _check(run_kernel(batch, gpu, want=(True, True, True, False), mask=gb[..., 0]), batch)


def run_kernel_output(c, gpu, mask):
    from dirt_amd import shading
    kw = {k: v for k, v in c.kw.items() if k != 'filter'}
    return shading.environment_background(_dev(gpu, c.levels[0]), _dev(gpu, c.M), c.size, mask=mask, intensity=_dev(gpu, c.intensity), filter=c.kw['filter'], **kw)


WANTS = [(True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True), (True, True, True, True),
         (False, False, False, False)]


@pytest.mark.gpu
@pytest.mark.parametrize('want', WANTS, ids=[''.join('emim'[i] if w else '-' for i, w in enumerate(want)) for want in WANTS])
def test_every_pattern_of_wanted_gradients(gpu, want):
    for name in ('rotation-2', 'batch:scene:shared:scene'):
        c = case(name)
        got = run_kernel(c, gpu, want)
        assert [k for k in R.KINDS[1:] if k in got] == [k for k, w in zip(R.KINDS[1:], want) if w]
        _check(got, c)


@pytest.mark.gpu
def test_two_runs_agree_to_the_bit(gpu):
    """Everything but the environment's gradient, which is summed with float atomics"""
    for name in ('footprint', 'batch:shared:shared:scene', 'batch:scene:scene:shared'):
        a, b = run_kernel(case(name), gpu), run_kernel(case(name), gpu)
        for k in ('out', 'd_matrix', 'd_intensity', 'd_mask'):
            assert np.array_equal(a[k], b[k]), (name, k)


@pytest.mark.gpu
def test_c_abi_with_guard_values_around_every_output(gpu, lib):
    """The entry points called as C would, every output and the scratch inside a larger buffer of a guard value: nothing outside is written"""
    from dirt_amd import _lib
    c = case('batch-footprint')
    levels = len(c.levels)
    env, M, I, m, go = (_dev(gpu, x) for x in (R.pack(c.levels), c.M, np.broadcast_to(c.intensity, (1, 3)).copy(), c.mask, c.go))
    pad, guard = 37, -77.25
    n = 3 * 17 * 19

    def guarded(count):
        return torch.full((count + 2 * pad,), guard, dtype=torch.float32, device=gpu)

    def inner(t, count):
        assert (t[:pad] == guard).all() and (t[pad + count:] == guard).all()
        return t[pad:pad + count]

    out, d_env, d_M, d_I, d_m = guarded(n * 3), guarded(env.numel()), guarded(48), guarded(3), guarded(n)
    nbytes = lib.dirt_background_scratch_bytes(3, 17, 19)
    scratch = guarded(nbytes // 4)
    at = lambda t: t.data_ptr() + 4 * pad   # noqa: E731
    tail = (3, 17, 19, 12, levels, 3, 1, 3, 1, 2, 0., float(np.float32(c.kw['lod_bias'])), _lib.BACKGROUND_FOOTPRINT, None)
    _lib.check(lib.dirt_background_forward(env.data_ptr(), M.data_ptr(), I.data_ptr(), m.data_ptr(), at(out), *tail))
    _lib.check(lib.dirt_background_backward(env.data_ptr(), M.data_ptr(), I.data_ptr(), m.data_ptr(), go.data_ptr(), at(d_env), at(d_M), at(d_I), at(d_m),
                                            at(scratch), nbytes, *tail))
    torch.cuda.synchronize()
    inner(scratch, nbytes // 4)
    packed = Case(c.levels, 'packed', c.M, c.size, c.mask, c.intensity, c.kw, 81)
    assert np.array_equal(packed.go, c.go)
    got = {'out': inner(out, n * 3).cpu().numpy().reshape(3, 17, 19, 3), 'd_environment': inner(d_env, env.numel()).cpu().numpy(),
           'd_matrix': inner(d_M, 48).cpu().numpy().reshape(3, 4, 4), 'd_intensity': inner(d_I, 3).cpu().numpy(),
           'd_mask': inner(d_m, n).cpu().numpy().reshape(3, 17, 19)}
    _check(got, packed)


@pytest.mark.gpu
def test_a_captured_call_replays_on_a_new_cube_and_a_new_matrix(gpu):
    """The call and its backward make no host synchronisation: captured with torch.cuda.graph and replayed, the cube and the matrix
    rewritten in place before each replay; the environment's gradient is cleared by a kernel of the library on every replay"""
    from dirt_amd import shading
    c = case('lod-0.7')
    cube, M, I, m, go = (_dev(gpu, x) for x in (c.levels[0], c.M, c.intensity, c.mask, c.go))

    def step():
        leaves = [x.detach().requires_grad_(True) for x in (cube, M, I, m)]
        out = shading.environment_background(leaves[0], leaves[1], c.size, mask=leaves[3], intensity=leaves[2], filter='trilinear', lod=0.7)
        return (out.detach(),) + tuple(torch.autograd.grad(out, leaves, go))

    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for k in range(3):
        other = case('lod-0.7') if k == 2 else make(300 + k, (17, 19), filter='trilinear', lod=0.7, rotation=(3, 5)[k])
        with torch.no_grad():
            cube.copy_(_dev(gpu, other.levels[0]))
            M.copy_(_dev(gpu, other.M))
        graph.replay()
        torch.cuda.synchronize()
        got = dict(zip(('out', 'd_environment', 'd_matrix', 'd_intensity', 'd_mask'), (x.cpu().numpy() for x in captured)))
        if k == 2:
            _check(got, c)
        else:       # the incoming gradient is the first case's: not zero on this one's kinks, so the value alone
            ref = R.compose_batch(other.levels, other.M, other.size, mask=c.mask, intensity=c.intensity, **other.kw)
            assert R.ratios({'out': got['out']}, ref)['out'] <= KERNEL * F32['out']


def _load(folder, name):
    spec = importlib.util.spec_from_file_location('%s_%s' % (folder, name), os.path.join(ROOT, folder, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_end_to_end_behind_rasterise_deferred(gpu):
    """The example's shader at 64 x 48 -- `shade_gbuffer_ibl(clamp=None) + environment_background(pyramid, mask=...)` with the one
    shared pyramid, inside `rasterise_deferred` -- against the torch forms of both terms on the same G-buffer"""
    from dirt_amd import lighting, texture
    from dirt_amd.texture import CubePyramid
    ex = _load('examples', 'fit_environment_background_fused')
    W, H = 64, 48
    scene, brdf, env = ex.Scene(gpu), lighting.environment_brdf(ex.TABLE).to(gpu), ex.true_environment(ex.SIZE, gpu)
    kept = []
    image = ex.render(scene, env, brdf, W, H, keep=kept)
    assert image.shape == (H, W, 3)
    g = kept[0].detach().cpu()
    pyr, irradiance = ex.filtered(env)
    levels = [pyr.level(k).cpu() for k in range(pyr.levels)]
    at = lambda name, width: g[..., ex.LAYOUT[name]:ex.LAYOUT[name] + width].reshape(-1, width)   # noqa: E731
    m = g[..., ex.LAYOUT['mask']]
    lit = lighting.image_based_lighting(at('positions', 3), at('normals', 3), at('colors', 3), at('material', 2)[:, 0], at('material', 2)[:, 1],
                                        torch.tensor(ex.CAMERA), levels, irradiance.cpu(), brdf.cpu()).reshape(H, W, 3) * m[..., None]
    inverse = ex.clip_to_world(torch.zeros(3), W, H)
    behind = lighting.environment_background(CubePyramid(pyr.packed.cpu(), pyr.size, 3, pyr.levels), inverse, (H, W), mask=m, filter='trilinear')
    want = (lit + behind).clamp(0., 1.).numpy()
    got = image.detach().cpu().numpy()
    # the two float32 routes part where an index crosses a lattice line: nearly every pixel agrees to 1e-4 of the [0, 1] range,
    # every pixel to what one texel step can change
    err = np.abs(got - want).max(-1)
    assert (err <= 1e-4).mean() >= 0.98 and err.max() <= 0.05, ((err <= 1e-4).mean(), err.max())
    background = (m == 0).numpy()
    assert background.sum() >= 500 and (m == 1).sum() >= 500 and got[background].max() > 0.05
    assert np.abs(got - behind.numpy())[background].max() <= 1e-4      # behind the mesh the image is the environment itself
