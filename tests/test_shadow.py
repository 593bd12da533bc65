"""`shading.shadow_visibility` (dirt_shadow.hip), its torch form `lighting.shadow_visibility`, `shading.render_shadow_map` and
`matrices.orthographic_projection`, by the method of the fused stages: tests/shadow_reference.py restates the specification of
DESIGN.md §7h in float64; the float32 torch form's worst |f32 - ref64| / mass per kind of result over the cases of
`tolerance_cases` is the F32 table below (`python -m tests.shadow_reference` prints it), and the kernel gets KERNEL times that,
per element against the element's L1 mass.  An element of zero mass must be exact."""
import ctypes
import functools
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import shadow_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# python -m tests.shadow_reference
F32 = {'out': 7.56e-7, 'd_positions': 3.90e-5, 'd_normals': 2.93e-6, 'd_mask': 1.20e-6, 'd_maps': 8.95e-5, 'd_matrices': 3.64e-7}
KERNEL = 4     # the kernel's allowance over the float32 composition


def kernel_constants():
    text = lambda name: open(os.path.join(ROOT, 'dirt_amd', 'csrc', name)).read()   # noqa: E731
    find = lambda source, name: int(re.search(r'constexpr int %s = (\d+);' % name, source).group(1))   # noqa: E731
    return find(text('dirt_shadow.hip'), 'SHADOW_BLOCK'), find(text('dirt_shadow.hip'), 'SHADOW_ITER'), find(text('dirt_texture_common.h'), 'TEX_PATCH')


SHADOW_BLOCK, SHADOW_ITER, TEX_PATCH = kernel_constants()
SPAN = SHADOW_BLOCK * SHADOW_ITER      # pixels of one backward workgroup
FLAT = SPAN + 3                        # one full workgroup and a second with three pixels
TILE = 16                              # the side of a backward tile of an image


# ---- the cases: each a scene [rows x cols pixels, Cg] with its maps, matrices and arguments, built once

class Case:
    def __init__(self, shape, gbuffer, maps, mats, layout, kw, seed):
        self.shape, self.g, self.maps, self.mats, self.layout, self.kw = shape, gbuffer, maps, mats, layout, kw
        self.go = np.random.default_rng(seed).standard_normal((gbuffer.shape[0], maps.shape[0])).astype(np.float32)

    @property
    def args(self):
        return (self.g, self.maps, self.mats, self.layout), dict(self.kw, grad_out=self.go)

    @functools.cached_property
    def ref(self):
        args, kw = self.args
        return R.compose(*args, **kw)


def random_case(seed, shape, cg, layout, lights, hs, ws, kernel, normal_offset=0., softness=0.5, bias=0.02):
    rng = np.random.default_rng(seed)
    maps, mats = R.random_scene(rng, lights, hs, ws)
    kw = dict(kernel=kernel, bias=bias, softness=softness, normal_offset=normal_offset)
    g, _ = R.draw_off_kinks(rng, int(np.prod(shape)), cg, layout, maps, mats, kw)
    return Case(shape, g, maps, mats, layout, kw, seed + 1)


def grid_case(seed, shape, hs, ws, rows, cols, kernel, cg=5, layout=(1, None, 0), mats=None):
    """Pixels placed at given fractional (row, col) indices of one map under the identity matrix (clip = [p, 1]): every pixel in
    the penumbra (|Z|, |d| small against the softness 1), so that every texel of every window carries a gradient.  `mats`
    [L, 4, 4]: a map per matrix, each a scale of x and y about the map's centre (the same pixels, a smaller or larger box)."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    op, _, om = layout
    g = rng.standard_normal((n, cg)).astype(np.float32)
    rows, cols = np.broadcast_to(rows, shape).reshape(-1), np.broadcast_to(cols, shape).reshape(-1)
    g[:, op] = (cols + 0.5) * 2. / ws - 1.
    g[:, op + 1] = 1. - (rows + 0.5) * 2. / hs
    g[:, op + 2] = rng.uniform(-0.05, 0.05, n)
    if om is not None:
        g[:, om] = rng.uniform(0.5, 1., n)
    mats = np.eye(4, dtype=np.float32)[None] if mats is None else np.asarray(mats, dtype=np.float32)
    maps = rng.uniform(-0.2, 0.2, (len(mats), hs, ws)).astype(np.float32)
    kw = dict(kernel=kernel, bias=0.01, softness=1., normal_offset=0.)
    case = Case(shape, g, maps, mats, layout, kw, seed + 1)
    assert case.ref['kink'].min() >= R.OFF_KINKS
    return case


def patch_case(seed, last):
    """One 16 x 16 tile under kernel 1 whose pixels step evenly from texel 0.5 to texel `last` + 0.5 of a 48 x 48 map along both
    axes: its window box is (last + 2) rows of 40 columns"""
    steps = 0.5 + np.arange(TILE) * (38. / (TILE - 1))
    rsteps = 0.5 + np.arange(TILE) * (float(last) / (TILE - 1))
    return grid_case(seed, (TILE, TILE), 48, 48, rsteps[:, None], steps[None, :], 1)


def edge_case(seed, kernel, hs=6, ws=5):
    """Windows straddling each border and each corner of the map, windows wholly outside it on every side, and the inside"""
    r = np.array([-4.7, -2.6, -1.3, -0.4, 0.3, 2.6, hs - 1.7, hs - 0.6, hs + 0.3, hs + 1.4, hs + 3.7])
    c = np.array([-4.6, -2.7, -1.4, -0.3, 0.4, 2.3, ws - 1.6, ws - 0.7, ws + 0.4, ws + 1.3, ws + 3.6])
    return grid_case(seed, (len(r), len(c)), hs, ws, r[:, None], c[None, :], kernel)


LAYOUTS = {'mask-first': (10, (1, 4, 0)), 'reversed': (9, (6, 3, 2)), 'no-mask': (7, (0, 4, None)), 'wide': (257, (254, 100, 3)), 'tight': (7, (4, 0, 3))}


@functools.lru_cache(maxsize=None)
def case(name):
    if name == 'flat':
        return random_case(10, (FLAT,), 10, (1, 4, 0), 2, 16, 12, 3, normal_offset=0.05)
    if name == 'image':
        return random_case(20, (17, 19), 12, (7, 4, 0), 3, 9, 7, 5)
    if name.startswith('lights'):
        _, lights, kernel = name.split('-')
        return random_case(30 + 7 * int(lights) + int(kernel), (13, 21), 8, (1, 4, 0), int(lights), 11, 14, int(kernel), normal_offset=0.03 * (int(lights) % 2))
    if name.startswith('layout'):
        cg, layout = LAYOUTS[name.split(':')[1]]
        return random_case(70 + cg, (18, 17) if cg < 100 else (5, 7), cg, layout, 2, 8, 8, 3, normal_offset=-0.04)
    if name == 'map-1x1':
        return random_case(80, (17, 19), 8, (1, 4, 0), 2, 1, 1, 3)
    if name == 'map-5x3':
        return random_case(81, (FLAT,), 8, (1, 4, 0), 1, 5, 3, 5, normal_offset=0.1)
    if name == 'patch-fits':
        return patch_case(90, 38)          # 40 x 40 = TEX_PATCH texels
    if name == 'patch-past':
        return patch_case(91, 39)          # 41 x 40: the first size past it
    if name == 'patch-flat':
        c = patch_case(92, 20)
        return Case((TILE * TILE,), c.g, c.maps, c.mats, c.layout, c.kw, 93)
    if name.startswith('edges'):
        return edge_case(100, int(name.split('-')[1]))
    if name == 'normals':
        c = random_case(110, (FLAT,), 9, (0, 3, 6), 2, 10, 10, 3, normal_offset=0.08)
        g = c.g.copy()
        g[1::3, 3:6] *= np.random.default_rng(111).uniform(0.1, 30., (len(g[1::3]), 1)).astype(np.float32)   # unit (the even pixels), scaled, zero (every seventh)
        keep = R.compose(g, c.maps, c.mats, c.layout, masses=False, **c.kw)['kink'] >= R.OFF_KINKS
        g[~keep] = c.g[~keep]
        return Case(c.shape, g, c.maps, c.mats, c.layout, c.kw, 112)
    raise KeyError(name)


LIGHT_CASES = ['lights-%d-%d' % (lights, kernel) for lights in (1, 2, 3, 4) for kernel in (1, 3, 5)]
LAYOUT_CASES = ['layout:' + k for k in LAYOUTS]
SINGLE_CASES = ['flat', 'image'] + LIGHT_CASES + LAYOUT_CASES + ['map-1x1', 'map-5x3', 'patch-fits', 'patch-past', 'patch-flat', 'edges-1', 'edges-3',
                                                                 'edges-5', 'normals']


def tolerance_cases():
    from tests import test_shadow_edges      # (it imports this module: here, not at the top)
    return [case(name).args for name in SINGLE_CASES] + test_shadow_edges.tolerance_cases()


def _check(got, c, what=None):
    ref = c.ref
    worst = R.ratios(got, ref, c.layout, c.kw['normal_offset'])
    print({k: '%.2e' % v for k, v in worst.items()})
    for kind, x in worst.items():
        assert x <= KERNEL * F32[kind], (what, kind, x, KERNEL * F32[kind])
    assert R.exact_where_massless(got, ref), what
    if got.get('d_gbuffer') is not None:      # a pixel whose every window is lit, or in the umbra: no gradient to its point or its normal, to the bit
        op, on, om = c.layout
        flat = ref['flat']
        assert not got['d_gbuffer'][flat, op:op + 3].any() and (on is None or not got['d_gbuffer'][flat, on:on + 3].any()), what
    return worst


# ---- not GPU: the torch form, the hand cases, the refusals, the entry points

def test_the_patch_cases_stand_where_they_are_meant_to():
    """The window box of 'patch-fits' holds exactly TEX_PATCH texels, the one of 'patch-past' one column of 40 more"""
    for name, texels in (('patch-fits', 40 * 40), ('patch-past', 41 * 40)):
        c = case(name)
        rows = np.floor(((1. - c.g[:, 2]) * 48 / 2. - 0.5).astype(np.float64))
        cols = np.floor(((c.g[:, 1] + 1.) * 48 / 2. - 0.5).astype(np.float64))
        assert (rows.max() + 1 - rows.min() + 1) * (cols.max() + 1 - cols.min() + 1) == texels, name
    assert 40 * 40 == TEX_PATCH


@pytest.mark.parametrize('name', ['flat', 'image', 'lights-4-5', 'lights-3-1', 'layout:wide', 'map-1x1', 'edges-3', 'normals'])
def test_torch_form_against_the_restatement(name):
    """`lighting.shadow_visibility` in float64 and the float64 restatement, which is written as a mean of bilinear blends, agree
    to 1e-12 of the masses, value and gradients; massless elements exactly"""
    c = case(name)
    args, kw = c.args
    got = R.torch_form(*args, dtype=torch.float64, **kw)
    for kind, x in R.ratios(got, c.ref, c.layout, c.kw['normal_offset']).items():
        assert x <= 1e-12, (kind, x)
    assert R.exact_where_massless(got, c.ref)
    assert (c.ref['mass_d_maps'] > 0).any() and (c.ref['mass_d_matrices'] > 0).any()


def test_the_f32_table_is_what_the_float32_torch_form_gives():
    """The committed F32 figures bound the float32 torch form on `tolerance_cases` and are not slack: each within a factor 1.25"""
    worst = R.measure_f32(tolerance_cases())
    print({k: '%.3e' % v for k, v in worst.items()})
    for kind in R.KINDS:
        assert worst[kind] <= F32[kind] <= 1.25 * worst[kind] + 1e-12, (kind, worst[kind], F32[kind])


def _hand(points, maps, mats, **kw):
    from dirt_amd import lighting
    return lighting.shadow_visibility(torch.tensor(points, dtype=torch.float64), None, torch.tensor(maps, dtype=torch.float64),
                                      torch.tensor(mats, dtype=torch.float64), **kw)


def _ident():
    return np.eye(4)[None]


def _texel_point(row, col, hs, ws, depth=0.):
    """the point that the identity matrix sends to the fractional texel index (row, col) of an hs x ws map"""
    return [(col + 0.5) * 2. / ws - 1., 1. - (row + 0.5) * 2. / hs, depth]


def test_hand_cases_umbra_lit_penumbra():
    """A square occluder at depth -0.5 over texels 2..5 of an 8 x 8 map, the rest at the far plane 1; receivers at depth 0.5,
    softness 0.1: a comparison is 0 under the occluder and 1 beside it.  Kernel 3 at the centre of texel (3, 3) sees 9 occluded
    texel centres: umbra, 0.  At the centre of texel (0, 0): lit, 1.  ON the edge between columns 1 and 2 (col = 1.5, the middle
    of the window's fractions) at row 3.5: the three filter taps are at columns 0.5, 1.5, 2.5 with blends 0, 1/2, 1 of occluded
    texels -> v = 1 - (0 + 1/2 + 1) / 3 = 1/2; one texel further out (col = 0.5): taps at -0.5, 0.5, 1.5 -> 1 - (1/2) / 3 = 5/6."""
    Z = np.ones((1, 8, 8))
    Z[0, 2:6, 2:6] = -0.5
    pts = [_texel_point(3., 3., 8, 8, 0.5), _texel_point(0., 0., 8, 8, 0.5), _texel_point(3.5, 1.5, 8, 8, 0.5), _texel_point(3.5, 0.5, 8, 8, 0.5)]
    v = _hand(pts, Z, _ident(), kernel=3, softness=0.1)[:, 0]
    np.testing.assert_allclose(v.numpy(), [0., 1., 0.5, 5. / 6.], atol=1e-14)
    v1 = _hand(pts, Z, _ident(), kernel=1, softness=0.1)[:, 0]        # kernel 1: one bilinear blend
    np.testing.assert_allclose(v1.numpy(), [0., 1., 0.5, 1.], atol=1e-14)
    # the smooth comparison itself: a receiver a quarter of the softness behind the map has t = 1/4, s = 5/32
    v = _hand([_texel_point(3., 3., 8, 8, -0.5 + 0.025)], Z, _ident(), kernel=1, softness=0.1)[:, 0]
    np.testing.assert_allclose(v.numpy(), [0.25 * 0.25 * (3. - 0.5)], atol=1e-13)
    # the bias moves the map: t = 1/4 + 0.05 / 0.1 = 3/4
    v = _hand([_texel_point(3., 3., 8, 8, -0.5 + 0.025)], Z, _ident(), kernel=1, softness=0.1, bias=0.05)[:, 0]
    np.testing.assert_allclose(v.numpy(), [0.75 * 0.75 * (3. - 1.5)], atol=1e-13)


def test_hand_cases_off_map_texels_count_one_and_no_gradient_behind_the_light():
    """A map that shadows everything (depth -1 against receivers at 0).  Kernel 3 at the centre of the corner texel (0, 0) of a
    4 x 4 map: 4 of its 9 taps are on the map -> v = 5/9; at the centre of texel (-1, 1): the taps' rows are -2, -1, 0, of which
    row 0 is on the map -> 3 of 9 occluded, v = 6/9; two texels out, (-2.5, 1): the window's last row is -0.5 + ... -> the blends
    at row -1.5 + 1 = -0.5 see half of row 0: v = 1 - (3 * 1/2) / 9.  Wholly outside: 1.  A matrix whose w is -1 or 0: v = 1,
    and no gradient reaches the point, the map or the matrix; a NaN position likewise gives 1."""
    Z = -np.ones((1, 4, 4))
    pts = [_texel_point(0., 0., 4, 4), _texel_point(-1., 1., 4, 4), _texel_point(-1.5, 1., 4, 4), _texel_point(-2.5, 1., 4, 4), _texel_point(1., 6.5, 4, 4)]
    v = _hand(pts, Z, _ident(), kernel=3, softness=0.1)[:, 0]
    np.testing.assert_allclose(v.numpy(), [5. / 9., 6. / 9., 1. - 1.5 / 9., 1., 1.], atol=1e-14)
    from dirt_amd import lighting
    for w in (-1., 0.):
        M = torch.eye(4, dtype=torch.float64)[None].clone()
        M[0, 3, 3] = w
        M.requires_grad_(True)
        p = torch.tensor([_texel_point(1., 1., 4, 4), [float('nan'), 0., 0.]], dtype=torch.float64, requires_grad=True)
        Zt = torch.tensor(Z, requires_grad=True)
        out = lighting.shadow_visibility(p, None, Zt, M, kernel=3, softness=0.1)
        assert out.tolist() == [[1.], [1.]]
        out.sum().backward()
        assert not p.grad.any() and not Zt.grad.any() and not M.grad.any()
    nan = lighting.shadow_visibility(torch.tensor([[float('nan'), 0., 0.]], dtype=torch.float64), None, torch.tensor(Z), torch.eye(4, dtype=torch.float64)[None],
                                     kernel=3, softness=0.1)
    assert nan.tolist() == [[1.]]
    # the mask: an uncovered pixel is lit, a half-covered one is half way
    out = lighting.shadow_visibility(torch.tensor([_texel_point(1., 1., 4, 4)] * 3, dtype=torch.float64), None, torch.tensor(Z),
                                     torch.eye(4, dtype=torch.float64)[None], mask=torch.tensor([0., 0.5, 1.], dtype=torch.float64), kernel=1, softness=0.1)
    np.testing.assert_allclose(out[:, 0].numpy(), [1., 0.5, 0.], atol=1e-15)


def test_the_window_is_the_mean_of_bilinear_blends():
    """v at a fractional index is the mean over the kernel^2 texel offsets of the bilinear blend of the comparison there"""
    rng = np.random.default_rng(5)
    Z = rng.uniform(-0.3, 0.3, (1, 7, 6))
    for kernel in (1, 3, 5):
        h = (kernel - 1) // 2
        row, col, d = 3.3, 2.6, 0.05
        S = np.ones((40, 40))
        t = np.clip((Z[0] - d + 0.01) / 0.5 + 0.5, 0., 1.)
        S[10:17, 10:16] = t * t * (3. - 2. * t)
        fr, fc = row - np.floor(row), col - np.floor(col)
        total = 0.
        for i in range(-h, h + 1):
            for j in range(-h, h + 1):
                r, c = int(np.floor(row)) + i + 10, int(np.floor(col)) + j + 10
                total += (1 - fr) * (1 - fc) * S[r, c] + (1 - fr) * fc * S[r, c + 1] + fr * (1 - fc) * S[r + 1, c] + fr * fc * S[r + 1, c + 1]
        v = _hand([_texel_point(row, col, 7, 6, d)], Z, _ident(), kernel=kernel, softness=0.5, bias=0.01)
        np.testing.assert_allclose(v.numpy(), [[total / kernel ** 2]], atol=1e-14)


def test_gradcheck_in_float64():
    from dirt_amd import lighting
    c = case('lights-2-3')
    live = np.abs(c.ref['d_gbuffer'][:, 1:4]).sum(1) * (np.linalg.norm(c.g[:, 4:7], axis=1) > 0.5)      # (a zero normal: the normalisation's 1e-12 is below any step)
    idx = np.argsort(-live)[:6]      # pixels in a penumbra
    g = torch.tensor(c.g[idx], dtype=torch.float64)
    p, n, m = (g[:, 1:4].clone().requires_grad_(True), g[:, 4:7].clone().requires_grad_(True), g[:, 0].clone().requires_grad_(True))
    Z, M = torch.tensor(c.maps, dtype=torch.float64, requires_grad=True), torch.tensor(c.mats, dtype=torch.float64, requires_grad=True)
    f = lambda p, n, m, Z, M: lighting.shadow_visibility(p, n, Z, M, mask=m, kernel=3, bias=0.02, softness=0.5, normal_offset=0.07)   # noqa: E731
    assert torch.autograd.gradcheck(f, (p, n, m, Z, M), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_every_value_error_of_the_wrapper():
    from dirt_amd import shading
    g = torch.zeros(4, 5, 8)
    Z, M = torch.zeros(2, 6, 6), torch.eye(4).expand(2, 4, 4)
    ok = dict(positions=1, normals=4, mask=0, softness=0.1)

    def refused(text, *args, **kw):
        with pytest.raises(ValueError) as e:
            shading.shadow_visibility(*args, **kw)
        assert str(e.value) == text, str(e.value)

    refused('shadow_visibility expects gbuffer [H, W, Cg], [B, H, W, Cg] or [N, Cg], got (8,)', torch.zeros(8), Z, M, **ok)
    refused('shadow_visibility expects a float32 gbuffer, got torch.int32', g.int(), Z, M, **ok)
    refused('shadow_visibility expects shadow_maps to be a floating-point tensor [L, Hs, Ws] with 1 <= L <= 4 and no empty map, got (5, 6, 6)',
            g, torch.zeros(5, 6, 6), M, **ok)
    refused('shadow_visibility expects shadow_maps to be a floating-point tensor [L, Hs, Ws] with 1 <= L <= 4 and no empty map, got (2, 2, 6, 6)',
            g, torch.zeros(2, 2, 6, 6), M, **ok)
    refused('shadow_visibility expects shadow_maps to be a floating-point tensor [L, Hs, Ws] or [B, L, Hs, Ws] with 1 <= L <= 4 and no empty map, got (2, 0, 6)',
            g[None], torch.zeros(2, 0, 6), M, **ok)
    refused('shadow_visibility expects shadow_maps to be a floating-point tensor [L, Hs, Ws] with 1 <= L <= 4 and no empty map, got ()', g, None, M, **ok)
    refused('shadow_visibility expects light_matrices to be a floating-point tensor [2, 4, 4], a matrix per map, got (3, 4, 4)', g, Z, torch.zeros(3, 4, 4), **ok)
    refused('shadow_visibility expects light_matrices to be a floating-point tensor [2, 4, 4] or [B, 2, 4, 4], a matrix per map, got (4, 4)',
            g[None], Z, torch.eye(4), **ok)
    refused('shadow_visibility: 3 scenes of gbuffer, 2 of shadow_maps', torch.zeros(3, 4, 5, 8), torch.zeros(2, 2, 6, 6), M, **ok)
    refused('shadow_visibility: 3 scenes of gbuffer, 4 of light_matrices', torch.zeros(3, 4, 5, 8), Z, torch.zeros(4, 2, 4, 4), **ok)
    refused('light_matrices is on meta, the G-buffer on cpu', g, Z, M.to('meta'), **ok)
    refused('positions at channel 6 does not fit in the 8 channels of the G-buffer', g, Z, M, **dict(ok, positions=6))
    refused('normals (channel 2) overlaps positions (channel 1)', g, Z, M, **dict(ok, normals=2))
    refused('mask must be the index of a G-buffer channel, got 0.5', g, Z, M, **dict(ok, mask=0.5))
    refused('kernel must be 1, 3 or 5, got 2', g, Z, M, kernel=2, **ok)
    refused('kernel must be 1, 3 or 5, got True', g, Z, M, kernel=True, **ok)
    refused('softness must be > 0, got 0.0', g, Z, M, **dict(ok, softness=0.))
    refused('softness must have a finite float32 reciprocal, got 1e-40', g, Z, M, **dict(ok, softness=1e-40))
    refused('softness must have a finite float32 reciprocal, got 1e-50', g, Z, M, **dict(ok, softness=1e-50))
    refused("softness must be a finite number, got 'soft'", g, Z, M, **dict(ok, softness='soft'))
    refused('bias must be a finite number, got nan', g, Z, M, bias=float('nan'), **ok)
    refused('normal_offset must be a finite number, got inf', g, Z, M, normal_offset=float('inf'), **ok)
    refused('shadow_visibility: normal_offset=0.1 needs normals', g, Z, M, normal_offset=0.1, **dict(ok, normals=None))
    with pytest.raises(RuntimeError, match='dirt_amd.shading.shadow_visibility runs on an MI355X only; there is no CPU fallback'):
        shading.shadow_visibility(g, Z, M, **ok)
    with pytest.raises(TypeError):
        shading.shadow_visibility(g, Z, M, positions=1)       # softness has no default
    for text, args in (('render_shadow_map expects vertices [V, 3], got (3, 4)', (torch.zeros(3, 4), torch.zeros(1, 3).int(), torch.eye(4), 8, 1.)),
                       ('render_shadow_map expects light_matrix [4, 4], got (1, 4, 4)', (torch.zeros(3, 3), torch.zeros(1, 3).int(), torch.eye(4)[None], 8, 1.)),
                       ('size must be a positive int or (height, width), got 0', (torch.zeros(3, 3), torch.zeros(1, 3).int(), torch.eye(4), 0, 1.)),
                       ('size must be a positive int or (height, width), got (8, 2.5)', (torch.zeros(3, 3), torch.zeros(1, 3).int(), torch.eye(4), (8, 2.5), 1.)),
                       ("far must be a finite number, the clip z of the light's far plane, got inf",
                        (torch.zeros(3, 3), torch.zeros(1, 3).int(), torch.eye(4), 8, float('inf')))):
        with pytest.raises(ValueError) as e:
            shading.render_shadow_map(*args)
        assert str(e.value) == text, str(e.value)
    with pytest.raises(ValueError) as e:
        shading.render_shadow_map_batch(torch.zeros(2, 3, 3), torch.zeros(1, 3).int(), torch.zeros(3, 4, 4), 8, 1.)
    assert str(e.value) == 'render_shadow_map_batch expects light_matrices [4, 4] or [2, 4, 4], got (3, 4, 4)'
    with pytest.raises(ValueError) as e:
        shading.render_shadow_map_batch(torch.zeros(3, 3), torch.zeros(1, 3).int(), torch.eye(4), 8, 1.)
    assert str(e.value) == 'render_shadow_map_batch expects vertices [B, V, 3], got (3, 3)'


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_entry_points_are_declared_listed_and_built(lib):
    from dirt_amd import _lib, build, lighting
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dirt_hip.h')).read(), flags=re.S)
    for name in ('dirt_shadow_scratch_bytes', 'dirt_shadow_forward', 'dirt_shadow_backward'):
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert '#define DIRT_ABI_VERSION 4' in header and '#define DIRT_SHADOW_MAX_LIGHTS 4' in header
    assert _lib.SHADOW_MAX_LIGHTS == _lib.SHADE_PBR_MAX_LIGHTS == lighting.SHADOW_MAX_LIGHTS == 4 and _lib.SHADOW_KERNELS == lighting.SHADOW_KERNELS == (1, 3, 5)
    assert 'dirt_shadow.hip' in build.SOURCES and 'dirt_shadow.hip' not in build.PER_SOURCE_FLAGS
    tiles = lambda rows, cols: -(-rows // TILE) * -(-cols // TILE) if rows > 1 else -(-cols // SHADOW_BLOCK)   # noqa: E731
    assert lib.dirt_shadow_scratch_bytes(3, 17, 19, 2) == 3 * tiles(17, 19) * 2 * 16 * 4
    assert lib.dirt_shadow_scratch_bytes(1, 1, FLAT, 4) == 2 * 4 * 16 * 4
    for bad in ((-1, 4, 4, 1), (65536, 4, 4, 1), (1, -4, 4, 1), (1, 4, 4, 0), (1, 4, 4, 5), (1, 1 << 31, 4, 1)):
        assert lib.dirt_shadow_scratch_bytes(*bad) == 0, bad


FWD = dict(gbuffer=None, maps=None, matrices=None, out=None, scenes=1, pixels=10, Cg=8, off_positions=1, off_normals=4, off_mask=0, lights=2, Hs=6, Ws=6,
           map_scenes=1, matrix_scenes=1, kernel=3, bias=0., softness=0.1, normal_offset=0., stream=None)
REFUSALS = [
    (dict(scenes=-1), 'dirt_shadow_forward: negative sizes (scenes=-1 pixels=10)'),
    (dict(scenes=65536), 'dirt_shadow_forward: 65536 scenes, at most 65535'),
    (dict(pixels=(1 << 40) + 1), 'dirt_shadow_forward: 1099511627777 pixels per scene, at most 2^40'),
    (dict(scenes=3, pixels=1 << 40, map_scenes=3), 'dirt_shadow_forward: 3 x 1099511627776 pixels, at most 2^40'),
    (dict(Cg=0), 'dirt_shadow_forward: 0 G-buffer channels, 1..1024'),
    (dict(Cg=1025), 'dirt_shadow_forward: 1025 G-buffer channels, 1..1024'),
    (dict(lights=0), 'dirt_shadow_forward: 0 lights, 1..4'),
    (dict(lights=5), 'dirt_shadow_forward: 5 lights, 1..4'),
    (dict(Hs=0), 'dirt_shadow_forward: a map of 0 x 6 texels, 1 x 1 to 2^31 - 1 texels'),
    (dict(Hs=1 << 16, Ws=1 << 15), 'dirt_shadow_forward: a map of 65536 x 32768 texels, 1 x 1 to 2^31 - 1 texels'),
    (dict(map_scenes=2), 'dirt_shadow_forward: map_scenes=2 is neither 1 nor scenes=1'),
    (dict(matrix_scenes=0), 'dirt_shadow_forward: matrix_scenes=0 is neither 1 nor scenes=1'),
    (dict(kernel=2), 'dirt_shadow_forward: kernel=2 is none of 1, 3, 5'),
    (dict(softness=0.), 'dirt_shadow_forward: softness=0 is not a finite number > 0'),
    (dict(softness=float('nan')), 'dirt_shadow_forward: softness=nan is not a finite number > 0'),
    (dict(softness=float('inf')), 'dirt_shadow_forward: softness=inf is not a finite number > 0'),
    (dict(softness=1e-40), 'dirt_shadow_forward: softness=9.99995e-41 has no finite float32 reciprocal'),
    (dict(bias=float('inf')), 'dirt_shadow_forward: bias=inf is not finite'),
    (dict(normal_offset=float('nan')), 'dirt_shadow_forward: normal_offset=nan is not finite'),
    (dict(normal_offset=0.5, off_normals=-1), 'dirt_shadow_forward: normal_offset=0.5 needs the normals\' channels'),
    (dict(off_positions=6), 'dirt_shadow_forward: positions at channel 6 does not fit in 8 channels'),
    (dict(off_normals=3), 'dirt_shadow_forward: normals (channel 3) overlaps positions (channel 1)'),
    (dict(off_mask=5), 'dirt_shadow_forward: mask (channel 5) overlaps normals (channel 4)'),
    (dict(off_mask=-2), 'dirt_shadow_forward: mask at channel -2 does not fit in 8 channels'),
    (dict(), 'dirt_shadow_forward: gbuffer / maps / matrices / out is NULL'),
]


def test_c_refusals_come_before_any_device_work(lib):
    """Every refusal returns DIRT_E_INVALID_ARGUMENT with its sentence in dirt_last_error() -- on a machine without a GPU, with
    NULL pointers: nothing was dereferenced and nothing was launched.  The backward shares the checks and adds its own."""
    from dirt_amd import _lib
    for change, text in REFUSALS:
        a = dict(FWD, **change)
        assert lib.dirt_shadow_forward(*a.values()) == _lib.E_INVALID_ARGUMENT, change
        assert _lib.last_error() == text, (_lib.last_error(), text)
    assert lib.dirt_shadow_forward(*dict(FWD, pixels=0).values()) == 0 and _lib.last_error() == ''
    bwd = dict(gbuffer=None, maps=None, matrices=None, grad_out=None, grad_gbuffer=None, grad_maps=None, grad_matrices=None, scratch=None, scratch_bytes=0,
               scenes=1, rows=3, cols=4, **{k: FWD[k] for k in list(FWD)[6:]})
    one = ctypes.c_void_p(16)      # a pointer that is not NULL and is never dereferenced: every call below is refused first
    for change, text in [(dict(rows=-1), 'dirt_shadow_backward: bad pixel grid (rows=-1 cols=4)'),
                         (dict(rows=1 << 30, cols=1 << 30), 'dirt_shadow_backward: bad pixel grid (rows=1073741824 cols=1073741824)'),
                         (dict(kernel=4), 'dirt_shadow_backward: kernel=4 is none of 1, 3, 5'),
                         (dict(lights=9), 'dirt_shadow_backward: 9 lights, 1..4'),
                         (dict(softness=1e-40), 'dirt_shadow_backward: softness=9.99995e-41 has no finite float32 reciprocal'),
                         (dict(grad_gbuffer=one), 'dirt_shadow_backward: gbuffer / maps / matrices / grad_out is NULL'),
                         (dict(grad_gbuffer=one, rows=1, cols=1 << 40), 'dirt_shadow_backward: pixel grid too large (rows=1 cols=1099511627776)'),
                         (dict(gbuffer=one, maps=one, matrices=one, grad_out=one, grad_matrices=one),
                          'dirt_shadow_backward: scratch is NULL or smaller than dirt_shadow_scratch_bytes (0 < 128)'),
                         (dict(gbuffer=one, maps=one, matrices=one, grad_out=one, grad_matrices=one, scratch=ctypes.c_void_p(18), scratch_bytes=128),
                          'dirt_shadow_backward: scratch is not 4-byte aligned')]:
        a = dict(bwd, **change)
        assert lib.dirt_shadow_backward(*a.values()) == _lib.E_INVALID_ARGUMENT, change
        assert _lib.last_error() == text, (_lib.last_error(), text)
    assert lib.dirt_shadow_backward(*bwd.values()) == 0 and _lib.last_error() == ''      # no gradient wanted: success, nothing is launched


def test_orthographic_projection_by_hand():
    """near 1, far 5, right 2, aspect 0.5: x / 2, y / 1, z -> -2 z / 4 - 6 / 4, w = 1; the box's corners go to the clip cube's"""
    from dirt_amd import matrices
    M = matrices.orthographic_projection(1., 5., 2., 0.5)
    assert M.tolist() == [[0.5, 0., 0., 0.], [0., 1., 0., 0.], [0., 0., -0.5, 0.], [0., 0., -1.5, 1.]]
    corners = torch.tensor([[2., 1., -1., 1.], [-2., -1., -5., 1.], [0., 0., -3., 1.]])
    assert (corners @ M).tolist() == [[1., 1., -1., 1.], [-1., -1., 1., 1.], [0., 0., 0., 1.]]
    batch = matrices.orthographic_projection(torch.tensor([1., 2.]), 6., 2., 1.)
    assert batch.shape == (2, 4, 4) and batch[1, 2, 2] == -0.5 and batch[1, 3, 2] == -2.
    near = torch.tensor(1., dtype=torch.float64, requires_grad=True)
    matrices.orthographic_projection(near, 5., 2., 0.5)[3, 2].backward()
    assert abs(float(near.grad) - (-10. / 16.)) < 1e-15          # d (-(f + n) / (f - n)) / d n = -2 f / (f - n)^2


def _quad_scene():
    """A tilted planar quad over part of the map and a perspective light: (vertices [4, 3], faces [2, 3], matrix [4, 4])"""
    from dirt_amd import matrices
    v = np.array([[-0.9, -0.7, 0.29], [0.8, -0.8, -0.4], [0.9, 0.75, -0.285], [-0.7, 0.6, 0.34]], np.float32)      # on the plane z = -0.4 x + 0.1 y
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    M = matrices.compose(matrices.translation(torch.tensor([0., 0., -3.])), matrices.perspective_projection(1., 6., 0.4, 1.))
    return v, f, M


def test_render_shadow_map_operands_against_the_oracle(oracle):
    """What `render_shadow_map` hands to the rasteriser, drawn by the oracle on an 8 x 8 map: every covered texel holds the clip
    z of the surface point that the look-up's own formula sends to that texel's centre (the quad is planar: the depth is the
    plane's, found by least squares over the vertices), every other texel `far`; the row order is the look-up's, not its flip."""
    from dirt_amd import shading
    v, f, M = _quad_scene()
    background, clip, depth = shading._shadow_map_operands(torch.from_numpy(v), M, 8, 6.)
    assert background.shape == (8, 8, 1) and (background == 6.).all() and clip.shape == (4, 4) and torch.equal(depth, clip[:, 2:3])
    image = oracle.forward(background.numpy()[None], clip.numpy()[None], depth.numpy()[None], f[None])[0, ..., 0]
    covered = image != 6.
    assert 20 <= covered.sum() < 64
    # clip z as an affine function of (x / w, y / w) is not exact under perspective; 1 / w and z / w are: fit those
    c = clip.numpy().astype(np.float64)
    A = np.stack([c[:, 0] / c[:, 3], c[:, 1] / c[:, 3], np.ones(4)], 1)
    inv_w, z_w = np.linalg.lstsq(A, 1. / c[:, 3], rcond=None)[0], np.linalg.lstsq(A, c[:, 2] / c[:, 3], rcond=None)[0]
    rows, cols = np.nonzero(covered)
    ndc = np.stack([(cols + 0.5) * 2. / 8 - 1., 1. - (rows + 0.5) * 2. / 8, np.ones(len(rows))], 1)
    expect = (ndc @ z_w) / (ndc @ inv_w)
    np.testing.assert_allclose(image[rows, cols], expect, rtol=0, atol=2e-5)
    flipped = (np.stack([ndc[:, 0], -ndc[:, 1], ndc[:, 2]], 1) @ z_w) / (np.stack([ndc[:, 0], -ndc[:, 1], ndc[:, 2]], 1) @ inv_w)
    assert np.abs(image[rows, cols] - flipped).max() > 0.05


# ---- GPU

def _dev(gpu, a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(gpu)


def _run(gpu, c, want=(True, True, True), shape=None, scenes=None):
    """The kernel on a case (or, `scenes`: on a list of cases as a batch, each operand of (gbuffer, maps, matrices) per scene where
    the list's entry says so) -> the keys of `compose`, as numpy"""
    from dirt_amd import shading
    shape = shape or c.shape
    op, on, om = c.layout
    g = _dev(gpu, c.g.reshape(shape + (-1,))).requires_grad_(want[0])
    Z, M = _dev(gpu, c.maps).requires_grad_(want[1]), _dev(gpu, c.mats).requires_grad_(want[2])
    out = shading.shadow_visibility(g, Z, M, positions=op, normals=on, mask=om, **c.kw)
    res = {'out': out.detach().cpu().numpy().reshape(-1, c.maps.shape[0])}
    leaves = [x for x, w in zip((g, Z, M), want) if w]
    if leaves:
        grads = iter(torch.autograd.grad(out, leaves, _dev(gpu, c.go.reshape(shape + (-1,)))))
        for key, w in zip(('d_gbuffer', 'd_maps', 'd_matrices'), want):
            res[key] = next(grads).cpu().numpy() if w else None
        if res['d_gbuffer'] is not None:
            res['d_gbuffer'] = res['d_gbuffer'].reshape(c.g.shape)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize('name', SINGLE_CASES)
def test_kernel_against_the_restatement(gpu, name):
    """Value and every gradient within KERNEL x F32 of the float64 restatement, massless elements exact: a flat list of one
    backward workgroup's span + 3, a 17 x 19 image, 1..4 lights x kernels 1, 3, 5, every layout (Cg = 257 too), maps of 1 x 1
    and 5 x 3, a tile whose box just fits the LDS patch, the first size past it and the flat form, windows over every border and
    corner, wholly outside and behind the light, unit, scaled and zero normals"""
    c = case(name)
    got = _run(gpu, c)
    _check(got, c, name)
    if name.startswith('layout'):       # every channel no attribute uses: an exact zero
        op, on, om = c.layout
        used = set(range(op, op + 3)) | set(range(on, on + 3)) | ({om} if om is not None else set())
        rest = [ch for ch in range(c.g.shape[1]) if ch not in used]
        assert not got['d_gbuffer'][:, rest].any()


@pytest.mark.gpu
@pytest.mark.parametrize('want', [(True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True),
                                  (False, True, True), (False, False, False)])
@pytest.mark.parametrize('name', ['flat', 'image'])
def test_every_pattern_of_wanted_gradients(gpu, name, want):
    c = case(name)
    got = _run(gpu, c, want)
    assert [got.get(k) is not None for k in ('d_gbuffer', 'd_maps', 'd_matrices')] == list(want)
    _check(got, c, (name, want))


@pytest.mark.gpu
@pytest.mark.parametrize('shared', [(True, True), (False, False), (True, False), (False, True)])
def test_a_batch_with_shared_and_per_scene_maps_and_matrices(gpu, shared):
    """B = 3 scenes of 17 x 19 pixels: a map set or a matrix set shared by the scenes gets the sum of the scenes' gradients (the
    matrices': in scene order, the same bits on every run), one per scene its scene's"""
    from dirt_amd import shading
    base = case('image')
    share_maps, share_mats = shared
    rng = np.random.default_rng(200)
    scenes = []
    for b in range(3):
        maps, mats = (base.maps, base.mats)
        if b and not share_maps:
            maps = R.random_scene(rng, 3, 9, 7)[0]
        if b and not share_mats:
            mats = R.random_scene(rng, 3, 9, 7)[1]
        g = base.g if b == 0 else R.draw_off_kinks(rng, 17 * 19, 12, base.layout, maps, mats, base.kw)[0]
        scenes.append(Case(base.shape, g, maps, mats, base.layout, base.kw, 210 + b))
    op, on, om = base.layout
    g = _dev(gpu, np.stack([s.g.reshape(17, 19, -1) for s in scenes])).requires_grad_(True)
    Z = _dev(gpu, base.maps if share_maps else np.stack([s.maps for s in scenes])).requires_grad_(True)
    M = _dev(gpu, base.mats if share_mats else np.stack([s.mats for s in scenes])).requires_grad_(True)
    out = shading.shadow_visibility(g, Z, M, positions=op, normals=on, mask=om, **base.kw)
    assert out.shape == (3, 17, 19, 3)
    dg, dZ, dM = (x.cpu().numpy() for x in torch.autograd.grad(out, (g, Z, M), _dev(gpu, np.stack([s.go.reshape(17, 19, -1) for s in scenes]))))
    total = lambda key: {key: sum(s.ref[key] for s in scenes), 'mass_' + key: sum(s.ref['mass_' + key] for s in scenes)}   # noqa: E731
    for b, s in enumerate(scenes):
        got = {'out': out[b].detach().cpu().numpy().reshape(-1, 3), 'd_gbuffer': dg[b].reshape(s.g.shape), 'd_maps': None if share_maps else dZ[b],
               'd_matrices': None if share_mats else dM[b]}
        _check(got, s, b)
    if share_maps:
        assert R.ratios({'d_maps': dZ}, total('d_maps'), base.layout)['d_maps'] <= KERNEL * F32['d_maps']
    if share_mats:
        assert R.ratios({'d_matrices': dM}, total('d_matrices'), base.layout)['d_matrices'] <= KERNEL * F32['d_matrices']


@pytest.mark.gpu
def test_two_runs_give_the_same_bits_in_the_gbuffer_and_matrix_gradients(gpu):
    for name in ('image', 'flat', 'patch-past'):
        a, b = _run(gpu, case(name)), _run(gpu, case(name))
        assert np.array_equal(a['out'], b['out']) and np.array_equal(a['d_gbuffer'], b['d_gbuffer']) and np.array_equal(a['d_matrices'], b['d_matrices'])


@pytest.mark.gpu
def test_c_abi_with_guard_values_around_every_output(gpu, lib):
    """The entry points called as C would, every output inside a larger buffer of a guard value: nothing outside is written"""
    from dirt_amd import _lib
    c = case('image')
    (hs, ws), lights, n, cg = c.maps.shape[1:], c.maps.shape[0], c.g.shape[0], c.g.shape[1]
    op, on, om = c.layout
    g, Z, M, go = (_dev(gpu, x) for x in (c.g, c.maps, c.mats, c.go))
    pad, guard = 37, -77.25

    def guarded(count):
        return torch.full((count + 2 * pad,), guard, dtype=torch.float32, device=gpu)

    def inner(t, count):
        assert (t[:pad] == guard).all() and (t[pad + count:] == guard).all()
        return t[pad:pad + count]

    out, dg, dZ, dM = guarded(n * lights), guarded(n * cg), guarded(Z.numel()), guarded(M.numel())
    nbytes = lib.dirt_shadow_scratch_bytes(1, 17, 19, lights)
    scratch = guarded(nbytes // 4)
    at = lambda t: t.data_ptr() + 4 * pad   # noqa: E731
    tail = (cg, op, on, om, lights, hs, ws, 1, 1, c.kw['kernel'], c.kw['bias'], c.kw['softness'], c.kw['normal_offset'], None)
    _lib.check(lib.dirt_shadow_forward(g.data_ptr(), Z.data_ptr(), M.data_ptr(), at(out), 1, n, *tail))
    _lib.check(lib.dirt_shadow_backward(g.data_ptr(), Z.data_ptr(), M.data_ptr(), go.data_ptr(), at(dg), at(dZ), at(dM), at(scratch), nbytes, 1, 17, 19, *tail))
    torch.cuda.synchronize()
    inner(scratch, nbytes // 4)
    got = {'out': inner(out, n * lights).cpu().numpy().reshape(n, lights), 'd_gbuffer': inner(dg, n * cg).cpu().numpy().reshape(n, cg),
           'd_maps': inner(dZ, Z.numel()).cpu().numpy().reshape(c.maps.shape), 'd_matrices': inner(dM, M.numel()).cpu().numpy().reshape(c.mats.shape)}
    _check(got, c)


@pytest.mark.gpu
def test_a_captured_lookup_replays_on_a_new_map(gpu):
    """The look-up and its backward make no host synchronisation: captured with torch.cuda.graph and replayed, the map rewritten
    in place before each replay; the maps' gradient is cleared by a kernel of the library on every replay"""
    from dirt_amd import shading
    c = case('image')
    op, on, om = c.layout
    g, Z, M, go = (_dev(gpu, x) for x in (c.g.reshape(17, 19, -1), c.maps, c.mats, c.go.reshape(17, 19, -1)))

    def step():
        leaves = [x.detach().requires_grad_(True) for x in (g, Z, M)]
        out = shading.shadow_visibility(*leaves, positions=op, normals=on, mask=om, **c.kw)
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
    rng = np.random.default_rng(300)
    for k in range(3):
        maps = c.maps if k == 2 else R.random_scene(rng, 3, 9, 7)[0]
        with torch.no_grad():
            Z.copy_(_dev(gpu, maps))
        graph.replay()
        torch.cuda.synchronize()
        got = dict(zip(('out', 'd_gbuffer', 'd_maps', 'd_matrices'), (x.cpu().numpy() for x in captured)))
        got['out'], got['d_gbuffer'] = got['out'].reshape(-1, 3), got['d_gbuffer'].reshape(c.g.shape)
        if k == 2:
            _check(got, c)
        else:       # off the reference's kinks no longer: the value alone, and the texels no window touches
            ref = R.compose(c.g, maps, c.mats, c.layout, **c.kw)
            assert R.ratios({'out': got['out']}, ref, c.layout)['out'] <= KERNEL * F32['out']


def _load(folder, name):
    spec = importlib.util.spec_from_file_location('%s_%s' % (folder, name), os.path.join(ROOT, folder, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_render_shadow_map_against_the_oracle(gpu, oracle):
    """`render_shadow_map` and its batch form on the GPU equal the oracle's drawing of the same operands (8 x 8 and 24 x 16)"""
    from dirt_amd import shading
    v, f, M = _quad_scene()
    for size in (8, (24, 16)):
        background, clip, depth = shading._shadow_map_operands(torch.from_numpy(v), M, size, 6.)
        expect = oracle.forward(background.numpy()[None], clip.numpy()[None], depth.numpy()[None], f[None])[0, ..., 0]
        got = shading.render_shadow_map(_dev(gpu, v), _dev(gpu, f), M.to(gpu), size, 6.)
        np.testing.assert_allclose(got.cpu().numpy(), expect, rtol=0, atol=1e-5)
        both = shading.render_shadow_map_batch(_dev(gpu, np.stack([v, v * 0.8])), _dev(gpu, f), M.to(gpu), size, 6.)
        np.testing.assert_allclose(both[0].cpu().numpy(), expect, rtol=0, atol=1e-5)
        assert both.shape == (2,) + expect.shape and (both[1] != 6.).sum() < (both[0] != 6.).sum()
    vg = _dev(gpu, v).requires_grad_(True)
    Mg = M.to(gpu).requires_grad_(True)
    shading.render_shadow_map(vg, _dev(gpu, f), Mg, 8, 6.).sum().backward()
    assert vg.grad.abs().sum() > 0 and Mg.grad.abs().sum() > 0


@pytest.mark.gpu
def test_end_to_end_floor_and_box(gpu, oracle):
    """The example's scene: the map from `render_shadow_map`, the G-buffer from `rasterise`, the look-up on the GPU -- against the
    oracle's drawing of the map fed to the float64 restatement on the same G-buffer.  The floor under the box is dark (< 0.02),
    the box's lit top reads 1 to the rounding of the window's sum (no self-shadow at the example's bias, softness and normal
    offset), and so does the floor away from the box."""
    import dirt_amd
    from dirt_amd import shading
    ex = _load('examples', 'fit_light_shadow_fused')
    vertices, faces, normals, colors = ex.build_scene()
    W, H = 128, 96
    direction = torch.tensor([0.45, -0.8, -0.35])
    M = ex.light_matrix(direction)
    background, clip, depth = shading._shadow_map_operands(torch.from_numpy(vertices), M, ex.MAP_SIZE, 1.)
    map_ref = oracle.forward(background.numpy()[None], clip.detach().numpy()[None], depth.detach().numpy()[None], faces[None])[0, ..., 0]
    v, f = _dev(gpu, vertices), _dev(gpu, faces)
    shadow_map = shading.render_shadow_map(v, f, M.to(gpu), ex.MAP_SIZE, 1.)
    np.testing.assert_allclose(shadow_map.cpu().numpy(), map_ref, rtol=0, atol=1e-5)
    v4 = torch.cat([v, torch.ones_like(v[:, :1])], 1)
    attributes = torch.cat([torch.ones_like(v[:, :1]), _dev(gpu, colors), _dev(gpu, normals), v], 1)
    gbuffer = dirt_amd.rasterise(torch.zeros(H, W, 10, device=gpu), v4 @ ex.camera_matrix(W, H, gpu), attributes, f)
    kw = dict(kernel=3, bias=ex.BIAS, softness=ex.SOFTNESS, normal_offset=ex.NORMAL_OFFSET)
    vis = shading.shadow_visibility(gbuffer, shadow_map[None], M.to(gpu)[None], positions=7, normals=4, mask=0, **kw)[..., 0].cpu().numpy()
    g = gbuffer.cpu().numpy().reshape(-1, 10)
    ref = R.compose(g, map_ref[None], M.numpy()[None], (7, 4, 0), **kw)
    off = ref['kink'] >= R.OFF_KINKS
    assert off.mean() > 0.8
    assert np.abs(vis.reshape(-1) - ref['out'][:, 0])[off].max() <= 1e-3      # the two maps differ by 1e-5 of a softness of 0.02
    pos, nrm, mask = g[:, 7:10], g[:, 4:7], g[:, 0]
    d = (direction / direction.norm()).numpy()
    floor = (mask > 0.999) & (nrm[:, 1] > 0.999) & (np.abs(pos[:, 1]) < 1e-4)
    # the box's shadow on the floor: its footprint |x|, |z| <= 0.6 at height y lands y d_xz / -d_y further along the light; the
    # footprint of the box's middle (y = 1.1) covers the square of side 0.3 around its centre with 0.45 to spare on every side,
    # three times the reach of the 3 x 3 window (2 texels of 8 / 128)
    cx, cz = 1.1 * d[0] / -d[1], 1.1 * d[2] / -d[1]
    under = floor & (np.abs(pos[:, 0] - cx) < 0.15) & (np.abs(pos[:, 2] - cz) < 0.15)
    top = (mask > 0.999) & (np.abs(pos[:, 1] - 1.6) < 1e-4) & (np.abs(pos[:, 0]) < 0.5) & (np.abs(pos[:, 2]) < 0.5)
    far = floor & (pos[:, 0] < -1.) & (np.abs(pos[:, 2]) < 2.5)      # the shadow falls towards +x
    assert under.sum() >= 10 and top.sum() >= 10 and far.sum() >= 10
    # "reads 1": to the rounding of the window's sum, KERNEL x F32 of the mass 1 + m (1 + v) = 3 of a covered, lit pixel
    lit = KERNEL * F32['out'] * 3.
    assert vis.reshape(-1)[under].max() < 0.02 and np.abs(vis.reshape(-1)[top] - 1.).max() <= lit and np.abs(vis.reshape(-1)[far] - 1.).max() <= lit


@pytest.mark.gpu
def test_the_example_recovers_the_light_direction(gpu):
    ex = _load('examples', 'fit_light_shadow_fused')
    losses, before, after = ex.fit(width=64, height=48, steps=30, device=gpu)
    assert losses[-1] < losses[0] and after < before
