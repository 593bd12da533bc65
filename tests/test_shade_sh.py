"""`dirt_amd.shading.shade_gbuffer_sh` (dirt_shade_sh.hip) and `dirt_amd.lighting.spherical_harmonics` against the restatement
of tests/shade_sh_reference.py: the lighting function composed on the CPU in float64, gradients by torch's autograd.  Every
comparison is per element, |gpu - ref64| <= tol * (L1 mass of the element's terms); an element of zero mass must equal the
reference exactly; the channels of d gbuffer no attribute uses must be exact zeros.

The tolerances are measured, not chosen: the float32 torch composition is run on `tolerance_cases()`, the random inputs of
the tests below, and its worst |f32 - ref64| / mass per kind of result is F32; the kernel, which may order a pixel's sums
differently, gets 4 x that.  Produced by

    python -m tests.shade_sh_reference

The hand-made kink pixels compare against the float32 composition on the same input by the same rule (bit equality between
two orders of a 27-term sum is not a property either has): the bound there is KERNEL x F32 of the float64 masses as well.
"""
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import shade_sh_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# worst |f32 - ref64| / mass of the float32 composition on tolerance_cases(), per kind of result (python -m tests.shade_sh_reference)
F32 = {'pixels': 5.21e-7, 'd_colors': 3.08e-7, 'd_normals': 2.92e-7, 'd_mask': 1.65e-7, 'd_params': 2.27e-7}
KERNEL = 4     # the kernel's allowance over the float32 composition
SWAP_FACTOR = 3.7e5 # test_swapped_scene_tables_show: the least (pixel movement / bound) over the scenes, recorded

LAMBERT = R.LAMBERT
CHANNEL_LAYOUTS = {   # name -> (Cg, layout); positions of the sample's layout and every other unused channel hold noise
    'c6': (6, dict(colors=0, normals=3, mask=None)),
    'c7': (7, dict(colors=4, normals=0, mask=3)),
    'c10': (10, dict(colors=4, normals=7, mask=0)),                  # examples/deferred.py: the mask first
    'c17': (17, dict(colors=14, normals=3, mask=0)),                 # colours in the last three channels
    'c255': (255, dict(colors=100, normals=252, mask=50)),
    'c256': (256, dict(colors=253, normals=0, mask=200)),
    'c257': (257, dict(colors=10, normals=254, mask=30)),            # the normals cross channel 256, in the last three
    'c1024': (1024, dict(colors=254, normals=1020, mask=1023)),      # the colours cross channel 256; the mask last
}
TENSOR_LAYOUTS = {    # the colours are a tensor: the G-buffer needs no colour channels
    't3': (3, dict(normals=0, mask=None)),
    't4a': (4, dict(normals=1, mask=0)),
    't4b': (4, dict(normals=0, mask=3)),
    't257': (257, dict(normals=254, mask=100)),
}
LAYOUTS = dict(CHANNEL_LAYOUTS, **TENSOR_LAYOUTS)


def kernel_constants():
    source = open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_shade_sh.hip')).read()
    return tuple(int(re.search(r'constexpr int %s = (\d+);' % name, source).group(1)) for name in ('SH_BLOCK', 'SH_ITER'))


SH_BLOCK, SH_ITER = kernel_constants()
SPAN = SH_BLOCK * SH_ITER      # pixels of one backward workgroup
FLAT = SPAN + 3                # one full workgroup and a second with three pixels: the reduce adds two rows


class Case:
    """Inputs of one comparison: pixels that stay off the clamp's edges, a coefficient table, a background, grad_out."""

    def __init__(self, seed, layout='c10', n=FLAT, K=9, normalize=False, clamp=(0., 1.), mask=True, band_scale=(1., 1., 1.), factor=1.,
                 batch=None, per_scene=(False, False)):
        self.cg, lay = LAYOUTS[layout]
        self.layout = dict(lay)
        if not mask:
            self.layout['mask'] = None
        self.tensor = 'colors' not in self.layout
        self.batch, self.per_scene = batch, per_scene
        self.n = n * (batch or 1)      # n: the pixels of one scene
        self.idx = np.repeat(np.arange(batch), n) if batch and any(per_scene) else None
        self.kw = dict(clamp=clamp, normalize=normalize, band_scale=tuple(band_scale))
        for attempt in range(3):     # a seed that misses draw_off_kinks' cap is replaced by seed + 50, + 100 (REPLACED_SEEDS)
            rng = np.random.default_rng(seed + 50 * attempt)
            self.coefficients = R.random_coefficients(rng, K, batch if batch and per_scene[0] else None, factor)
            self.kw['background'] = rng.uniform(0.1, 0.9, (batch, 3) if batch and per_scene[1] else (3,)).astype(np.float32)
            try:
                self.g, self.colors, self.share = R.draw_off_kinks(rng, self.n, self.cg, self.layout, self.coefficients, self.kw,
                                                                    tensor_colors=self.tensor, scene_index=self.idx)
            except AssertionError:
                continue
            self.seed = seed + 50 * attempt
            break
        else:
            raise AssertionError('seed %d: no draw under the cap' % seed)
        self.go = rng.standard_normal((self.n, 3)).astype(np.float32)

    def measure(self):
        return (self.g, self.coefficients, self.layout), dict(self.kw, colors=self.colors, grad_out=self.go, scene_index=self.idx)

    def reference(self):
        args, kw = self.measure()
        return R.compose(*args, **kw)


def _options():
    """K x normalize x clamp, the mask present in every second case, the Lambert band scale (with the table divided by pi, so
    that the pixels stay in range) in every third"""
    cases, i = {}, 0
    for K in (1, 4, 9):
        for normalize in (False, True):
            for cname, clamp in (('clamp', (0., 1.)), ('noclamp', None), ('narrow', (0.3, 0.6))):
                lambert = i % 3 == 0
                cases['K%d-%s-%s-%s-%s' % (K, 'unit' if not normalize else 'normalize', cname, 'mask' if i % 2 == 0 else 'nomask',
                                           'lambert' if lambert else 'plain')] = dict(
                    seed=5100 + i, K=K, normalize=normalize, clamp=clamp, mask=i % 2 == 0, band_scale=LAMBERT if lambert else (1., 1., 1.),
                    factor=1. / math.pi if lambert else 1.)
                i += 1
    return cases


def _layout_n(name):
    return FLAT if LAYOUTS[name][0] < 255 else SH_BLOCK + 3     # the wide ones: a full pass of the copy-out walk and three pixels


CASES = dict(
    {'pattern_channel': dict(seed=5000, layout='c10'), 'pattern_tensor': dict(seed=5001, layout='t4a', normalize=True),
     'outer_channel': dict(seed=5002, layout='c10', factor=2.5, normalize=True), 'outer_tensor': dict(seed=5003, layout='t4b', factor=2.5),
     'same_data': dict(seed=5004, layout='c10', normalize=True, band_scale=LAMBERT, factor=1. / math.pi)},
    **_options(),
    **{name: dict(seed=5200 + i, layout=name, n=_layout_n(name), normalize=i % 2 == 1, clamp=(0., 1.) if i % 3 else None)
       for i, name in enumerate(LAYOUTS)},
    **{'scenes_%d_%s' % (n, 'per_scene' if per else 'shared'): dict(seed=5300 + 2 * i + per, layout='c7', n=n, batch=3, per_scene=(per, per),
                                                                   normalize=bool(per))
       for i, n in enumerate((SPAN, SPAN + 1)) for per in (False, True)},
    **{'scenes_mixed': dict(seed=5310, layout='t4a', n=SPAN + 1, batch=3, per_scene=(True, False), K=4)})
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

def shade(case, dev, want=(True, True, True), g=None, colors=None, normals_only=False):
    """-> dict of the fused call's results on `case`: out and the gradients wanted of (G-buffer, parameters, colour tensor)"""
    from dirt_amd import shading
    want_g, want_p, want_c = want
    shape = (case.batch, case.n // case.batch, 1) if case.batch else (case.n,)
    g = torch.from_numpy(case.g).to(dev).reshape(shape + (case.cg,)) if g is None else g
    g = g.detach().requires_grad_(want_g)
    L = torch.from_numpy(case.coefficients).to(dev).requires_grad_(want_p)
    bg = torch.from_numpy(case.kw['background']).to(dev).requires_grad_(want_p)
    if case.tensor:
        col = (torch.from_numpy(case.colors).to(dev).reshape(shape + (3,)) if colors is None else colors).detach().requires_grad_(want_c)
    else:
        col = case.layout['colors'] if colors is None else colors
    out = shading.shade_gbuffer_sh(g, L, colors=col, normals=case.layout['normals'], mask=case.layout.get('mask'), background=bg,
                                   clamp=case.kw['clamp'], normalize=case.kw['normalize'], band_scale=case.kw['band_scale'])
    res = {'out': out.detach().reshape(-1, 3)}
    if out.requires_grad:
        out.backward(torch.from_numpy(case.go).to(dev).reshape(out.shape))
    if want_g:
        res['d_gbuffer'] = g.grad.reshape(-1, case.cg)
        sl = lambda k, w: slice(case.layout[k], case.layout[k] + w)   # noqa: E731
        res['d_normals'] = res['d_gbuffer'][:, sl('normals', 3)]
        res['d_mask'] = res['d_gbuffer'][:, sl('mask', 1)] if case.layout.get('mask') is not None else None
        if not case.tensor:
            res['d_colors'] = res['d_gbuffer'][:, sl('colors', 3)]
    if case.tensor and want_c and isinstance(col, torch.Tensor):
        res['d_colors'] = col.grad.reshape(-1, 3)
    if want_p:
        res['d_coefficients'], res['d_background'] = L.grad, bg.grad
    return res


def check(case, got, ref, what, factor=KERNEL):
    """The mass rule per kind of result, exact equality where the mass is zero, exact zeros in the unused channels."""
    worst = R.ratios(got, ref)
    print(what, ' '.join('%s %.2f' % (k, v / F32[k]) for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= factor * F32[k], '%s %s: |gpu - ref64| / mass = %.3e, allowed %.3e' % (what, k, v, factor * F32[k])
    for key, mass in (('out', 'mass_out'), ('d_colors', 'mass_colors'), ('d_normals', 'mass_normals'), ('d_mask', 'mass_mask'),
                      ('d_coefficients', 'mass_coefficients'), ('d_background', 'mass_background')):
        if got.get(key) is None:
            continue
        a, r, m = got[key].detach().cpu().double().reshape(ref[key].shape), ref[key], ref[mass]
        assert bool(torch.isfinite(a).all()), (what, key)
        assert torch.equal(a[m == 0], r[m == 0]), '%s %s: an element of zero mass differs' % (what, key)
    if got.get('d_gbuffer') is not None:
        unused = np.ones(case.cg, bool)
        for k, w in (('colors', 3), ('normals', 3), ('mask', 1)):
            if case.layout.get(k) is not None:
                unused[case.layout[k]:case.layout[k] + w] = False
        assert not bool(got['d_gbuffer'][:, torch.from_numpy(unused).to(got['d_gbuffer'].device)].any()), '%s: d gbuffer of an unused channel' % what


def compare(name, dev, want=(True, True, True)):
    case, ref = case_of(name)
    got = shade(case, dev, want)
    check(case, got, ref, name)
    return case, ref, got


# ---- CPU tests

def test_the_basis_is_orthonormal_over_the_sphere():
    """Gauss-Legendre in cos(theta) x uniform phi integrates the products of the nine functions (polynomials of degree <= 4 in
    x, y, z) exactly: the Gram matrix is the identity to 1e-12, which fixes the five constants independently of the kernel."""
    from dirt_amd import lighting
    t, wt = np.polynomial.legendre.leggauss(8)
    phi = 2. * np.pi * np.arange(16) / 16
    z = np.repeat(t, 16)
    s = np.sqrt(1. - z * z)
    n = np.stack([s * np.cos(np.tile(phi, 8)), s * np.sin(np.tile(phi, 8)), z], 1)
    w = np.repeat(wt, 16) * (2. * np.pi / 16)
    Y = lighting.sh_basis(torch.from_numpy(n)).numpy()
    assert Y.shape == (128, 9) and Y.dtype == np.float64
    gram = (Y * w[:, None]).T @ Y
    assert np.abs(gram - np.eye(9)).max() <= 1e-12
    assert abs(lighting.SH_C0 - 0.5 / math.sqrt(math.pi)) < 1e-15 and lighting.SH_BAND == (0, 1, 1, 1, 2, 2, 2, 2, 2)


def _numpy_sh(n, c, L, scale, normalize):
    """the specification of DESIGN.md §7b written out in numpy float64"""
    n = np.asarray(n, np.float64)
    if normalize:
        n = n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-12)
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    C0, C1, C2, C3, C4 = 0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396
    Y = np.stack([C0 + 0 * x, C1 * y, C1 * z, C1 * x, C2 * x * y, C2 * y * z, C3 * (3 * z * z - 1), C2 * x * z, C4 * (x * x - y * y)], -1)
    s = np.asarray([scale[0]] + [scale[1]] * 3 + [scale[2]] * 5)
    K = L.shape[-2]
    return Y, c * np.einsum('...k,...kj->...j', Y[..., :K] * s[:K], np.asarray(L, np.float64))


def test_sh_basis_and_spherical_harmonics_against_the_specification():
    from dirt_amd import lighting
    rng = np.random.default_rng(5400)
    n, c = rng.standard_normal((2, 7, 3)), rng.uniform(0., 1., (2, 7, 3))
    for K in (1, 4, 9):
        for L in (rng.standard_normal((K, 3)), rng.standard_normal((2, K, 3))):
            for normalize in (False, True):
                Y, want = _numpy_sh(n, c, L[:, None] if L.ndim == 3 else L, LAMBERT, normalize)
                got = lighting.spherical_harmonics(torch.from_numpy(n), torch.from_numpy(c), torch.from_numpy(L), band_scale=LAMBERT,
                                                   normalize=normalize)
                assert got.shape == (2, 7, 3) and np.abs(got.numpy() - want).max() <= 1e-14
                if not normalize:
                    assert np.abs(lighting.sh_basis(torch.from_numpy(n)).numpy() - Y).max() <= 1e-15
    # K = 1 and K = 4 are K = 9 with zero rows
    for K in (1, 4):
        L = rng.standard_normal((K, 3))
        padded = np.concatenate([L, np.zeros((9 - K, 3))])
        a = lighting.spherical_harmonics(torch.from_numpy(n), torch.from_numpy(c), torch.from_numpy(L))
        b = lighting.spherical_harmonics(torch.from_numpy(n), torch.from_numpy(c), torch.from_numpy(padded))
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match=re.escape('coefficients must have shape [K, 3] or [B, K, 3] with K in (1, 4, 9), got [5, 3]')):
        lighting.spherical_harmonics(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(5, 3))
    with pytest.raises(ValueError, match='band_scale must be 3 numbers, got 2'):
        lighting.spherical_harmonics(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 3), band_scale=(1., 2.))
    # the restatement's value is the specification's, a zero normal included
    g = rng.standard_normal((5, 7)).astype(np.float32)
    g[0, 4:7] = 0.
    L, bg = rng.standard_normal((9, 3)).astype(np.float32), rng.uniform(0., 1., 3).astype(np.float32)
    ref = R.compose(g, L, dict(colors=0, normals=4, mask=3), background=bg, clamp=None, normalize=True, band_scale=LAMBERT)
    _, lit = _numpy_sh(g[:, 4:7], g[:, 0:3].astype(np.float64), L, LAMBERT, True)
    assert np.abs(ref['pre'].numpy() - (lit * g[:, 3:4] + bg * (1. - g[:, 3:4].astype(np.float64)))).max() <= 1e-12


def test_the_float32_composition_stays_within_the_committed_figures():
    """F32 is what `python -m tests.shade_sh_reference` prints: measured again here on every case of this file (Case asserts
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


def test_the_cases_hold_what_their_names_say():
    assert (SH_BLOCK, SH_ITER) == (256, 4) and FLAT == 1027
    header = open(os.path.join(ROOT, 'include', 'dirt_hip.h')).read()
    assert '#define DIRT_SHADE_MAX_CHANNELS 1024' in header
    for name in ('outer_channel', 'outer_tensor'):     # the table x 2.5: a good share of the values beyond the clamp's upper edge
        case, ref = case_of(name)
        inside = float(((ref['pre'] > 0.) & (ref['pre'] < 1.)).double().mean())      # of the values, not of the pixels
        assert 0.3 < inside < 0.9, (name, inside)
    for name in ('pattern_channel', 'pattern_tensor'):
        case, ref = case_of(name)
        inside = float(((ref['pre'] > 0.) & (ref['pre'] < 1.)).all(1).double().mean())
        assert case.n == FLAT and inside > 0.9, (name, inside)
    for name in LAYOUTS:
        case, _ = case_of(name)
        assert case.g.shape == (case.n, LAYOUTS[name][0]) and (case.colors is None) == (name in CHANNEL_LAYOUTS)
    assert sorted(LAYOUTS[k][0] for k in CHANNEL_LAYOUTS) == [6, 7, 10, 17, 255, 256, 257, 1024]
    assert case_of('scenes_%d_per_scene' % SPAN)[0].coefficients.shape == (3, 9, 3)
    assert case_of('scenes_%d_shared' % (SPAN + 1))[0].n == 3 * (SPAN + 1)


def test_swapped_scene_tables_show():
    """With the coefficient tables of two scenes swapped, the restatement's pixels of a scene move by far more than the bound:
    a kernel that read (or summed into) a neighbour's table could not pass.  SWAP_FACTOR records the least movement / bound."""
    case, ref = case_of('scenes_%d_per_scene' % (SPAN + 1))
    args, kw = case.measure()
    swapped = R.compose(args[0], case.coefficients[[1, 0, 2]], args[2], **dict(kw, masses=False))
    per = case.n // 3
    factors = []
    for s in (0, 1):
        rows = slice(s * per, (s + 1) * per)
        moved = ((swapped['out'][rows] - ref['out'][rows]).abs() / ref['mass_out'][rows]).max()
        factors.append(float(moved) / (KERNEL * F32['pixels']))
        moved_p = ((swapped['d_coefficients'][s] - ref['d_coefficients'][s]).abs() / ref['mass_coefficients'][s]).max()
        assert float(moved_p) > 100 * KERNEL * F32['d_params']
    print('swap factor %.3g' % min(factors))
    assert min(factors) > 1000 and 0.5 * SWAP_FACTOR <= min(factors) <= 2. * SWAP_FACTOR


G = torch.zeros(4, 5, 10)
CPU = ' runs on an MI355X only; there is no CPU fallback'


def test_shade_gbuffer_sh_refuses_bad_arguments():
    from dirt_amd import shading
    L = torch.zeros(9, 3)

    def check_args(g=G, coefficients=L, colors=4, normals=7, mask=0, background=(0., 0., 0.), clamp=(0., 1.), normalize=False,
                   band_scale=(1., 1., 1.)):
        return shading._check_sh_arguments(g, coefficients, colors, normals, mask, background, clamp, normalize, band_scale)

    G4 = torch.zeros(2, 4, 5, 10)
    for kw, text in (
            (dict(coefficients=torch.zeros(5, 3)), 'coefficients must have shape [K, 3] or [B, K, 3] with K in (1, 4, 9), got [5, 3]'),
            (dict(coefficients=torch.zeros(9, 4)), 'coefficients must have shape [K, 3] or [B, K, 3] with K in (1, 4, 9), got [9, 4]'),
            (dict(coefficients=torch.zeros(27)), 'coefficients must have shape [K, 3] or [B, K, 3] with K in (1, 4, 9), got [27]'),
            (dict(coefficients=torch.zeros(2, 9, 3)),
             'coefficients [B, K, 3] need a [B, H, W, Cg] G-buffer with the same B, got [2, 9, 3] against a G-buffer [4, 5, 10]'),
            (dict(g=G4, coefficients=torch.zeros(3, 4, 3)),
             'coefficients [B, K, 3] need a [B, H, W, Cg] G-buffer with the same B, got [3, 4, 3] against a G-buffer [2, 4, 5, 10]'),
            (dict(coefficients=torch.zeros(9, 3, device='meta')), 'coefficients is on meta, the G-buffer on cpu'),
            (dict(coefficients=torch.zeros(9, 3, dtype=torch.int32)), 'coefficients must be a floating-point tensor, got torch.int32'),
            (dict(coefficients=[[0., 0., 0.]]), 'coefficients must be a floating-point tensor, got list'),
            (dict(g=G.to(torch.int32)), 'shade_gbuffer_sh expects a float32 gbuffer, got torch.int32'),
            (dict(colors=torch.zeros(4, 5, 4)),
             "colors as a tensor must have shape [4, 5, 3] (the G-buffer's [4, 5, 10] with 3 channels), got [4, 5, 4]"),
            (dict(colors=torch.zeros(4, 5, 3, dtype=torch.int64)), 'colors as a tensor must be floating-point, got torch.int64'),
            (dict(colors=torch.zeros(4, 5, 3, device='meta')), 'colors is on meta, the G-buffer on cpu'),
            (dict(colors=5), 'normals (channel 7) overlaps colors (channel 5)'),
            (dict(mask=8), 'mask (channel 8) overlaps normals (channel 7)'),
            (dict(normals=8), 'normals at channel 8 does not fit in the 10 channels of the G-buffer'),
            (dict(colors=1.5), 'colors must be the index of a G-buffer channel, got 1.5'),
            (dict(band_scale=(1., 2.)), 'band_scale must be 3 numbers, got 2'),
            (dict(band_scale=1.), 'band_scale must be 3 numbers, got 1.0'),
            (dict(band_scale=('a', 1., 1.)), "band_scale must be 3 numbers, got ('a', 1.0, 1.0)"),
            (dict(background=(1., 2.)), 'background must be 3 numbers, got 2'),
            (dict(background=torch.zeros(2, 3)), 'background must have shape [3], got [2, 3]'),
            (dict(clamp=(1., 0.)), 'clamp needs lo <= hi, got (1.0, 0.0)'),
            (dict(clamp=3.), 'clamp must be (lo, hi) or None, got 3.0')):
        with pytest.raises(ValueError) as e:
            check_args(**kw)
        assert str(e.value) == text, (kw, str(e.value))
    offsets, scale, lo, hi, flags, const, tensors = check_args(g=G4, coefficients=torch.ones(2, 4, 3), band_scale=LAMBERT, normalize=True,
                                                               background=(0.1, 0.2, 0.3))
    from dirt_amd import _lib
    assert offsets == [4, 7, 0] and scale == LAMBERT and (lo, hi) == (0., 1.) and flags == _lib.SHADE_CLAMP | _lib.SHADE_SH_NORMALIZE
    assert const == [0.] * 27 + [0.1, 0.2, 0.3] and [(s, tuple(t.shape)) for s, t in tensors] == [(0, (2, 12))]
    block = shading._splice_block(G4.device, const, tensors)
    assert block.shape == (2, 30) and bool((block[:, :12] == 1).all()) and not bool(block[:, 12:27].any())
    assert check_args(clamp=None)[2:5] == (0., 0., 0) and check_args(colors=torch.zeros(4, 5, 3))[0] == [-1, 7, 0]
    with pytest.raises(ValueError) as e:
        shading.shade_gbuffer_sh(torch.zeros(5), L, colors=0, normals=3)
    assert str(e.value) == 'shade_gbuffer_sh expects gbuffer [H, W, Cg], [B, H, W, Cg] or [N, Cg], got (5,)'
    for g in (G, G.to('meta')):
        with pytest.raises(RuntimeError) as e:
            shading.shade_gbuffer_sh(g, L.to(g.device), colors=4, normals=7)
        assert str(e.value) == 'dirt_amd.shading.shade_gbuffer_sh' + CPU


def test_the_function_is_exported_and_declared():
    import dirt
    import dirt.shading
    import dirt_amd
    from dirt_amd import _lib, build
    assert dirt.shading.shade_gbuffer_sh is dirt_amd.shading.shade_gbuffer_sh
    assert 'dirt_shade_sh.hip' in build.SOURCES and 'dirt_shade_sh.hip' not in build.PER_SOURCE_FLAGS
    header = open(os.path.join(ROOT, 'include', 'dirt_hip.h')).read()
    for symbol in ('dirt_shade_sh_scratch_bytes', 'dirt_shade_sh_forward', 'dirt_shade_sh_backward'):
        assert symbol in _lib.SYMBOLS and re.search(r'\b%s\(' % symbol, header)
    assert '#define DIRT_SHADE_SH_PARAMS %d\n' % _lib.SHADE_SH_PARAMS in header and _lib.SHADE_SH_PARAMS == 30
    assert '#define DIRT_SHADE_SH_NORMALIZE %du\n' % _lib.SHADE_SH_NORMALIZE in header and _lib.SHADE_SH_NORMALIZE == 4
    assert _lib.SHADE_SH_NORMALIZE not in (_lib.SHADE_CLAMP, _lib.SHADE_HAS_CAMERA) and _lib.ABI_VERSION == 4


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import _lib, build
    build.build_library()
    return _lib.load()


def test_c_entry_points_refuse_bad_arguments_without_a_device(lib):
    from dirt_amd import _lib
    one = ctypes.c_void_p(16)
    E = _lib.E_INVALID_ARGUMENT

    def fwd(g=one, c=None, p=one, out=one, scenes=1, pixels=64, cg=10, stride=0, oc=4, on=7, om=0, ps=1, lo=0., hi=1., flags=1):
        return lib.dirt_shade_sh_forward(g, c, p, out, scenes, pixels, cg, stride, oc, on, om, ps, 1., 1., 1., lo, hi, flags, None)

    def bwd(g=one, c=None, p=one, go=one, gg=one, gc=None, gp=one, scratch=one, nbytes=1 << 20, scenes=1, pixels=64, cg=10, stride=0, oc=4,
            on=7, om=0, ps=1, lo=0., hi=1., flags=1):
        return lib.dirt_shade_sh_backward(g, c, p, go, gg, gc, gp, scratch, nbytes, scenes, pixels, cg, stride, oc, on, om, ps, 1., 1., 1., lo, hi,
                                          flags, None)

    for who, call in (('dirt_shade_sh_forward', fwd), ('dirt_shade_sh_backward', bwd)):
        for kw, text in ((dict(cg=1025), '%s: 1025 G-buffer channels, 1..1024'), (dict(cg=0), '%s: 0 G-buffer channels, 1..1024'),
                         (dict(scenes=-1), '%s: negative sizes (scenes=-1 pixels=64)'), (dict(pixels=-5), '%s: negative sizes (scenes=1 pixels=-5)'),
                         (dict(scenes=65536), '%s: 65536 scenes, at most 65535'),
                         (dict(c=one, stride=2), '%s: color_stride=2, a pixel\'s colour is 3 floats'),
                         (dict(ps=2), '%s: param_scenes=2 is neither 1 nor scenes=1'),
                         (dict(flags=3), '%s: unknown flags 0x3'),
                         (dict(oc=8), '%s: colors at channel 8 does not fit in 10 channels'),
                         (dict(oc=-1), '%s: colors at channel -1 does not fit in 10 channels'),
                         (dict(on=5), '%s: normals (channel 5) overlaps colors (channel 4)'),
                         (dict(om=9), '%s: mask (channel 9) overlaps normals (channel 7)'),
                         (dict(om=10), '%s: mask at channel 10 does not fit in 10 channels'),
                         (dict(lo=1., hi=0.), '%s: clamp bounds lo=1 > hi=0')):
            assert call(**kw) == E, (who, kw)
            assert lib.dirt_last_error().decode() == text % who, (who, kw, lib.dirt_last_error())
        assert call(pixels=0) == 0 and call(scenes=0) == 0 and lib.dirt_last_error() == b''
        # with a colour tensor off_colors is not read, and the G-buffer may be three channels of normals
        assert call(c=one, stride=3, oc=-1, cg=3, on=0, om=-1, pixels=0) == 0
    assert fwd(out=None) == E and lib.dirt_last_error().decode() == 'dirt_shade_sh_forward: gbuffer / params / out is NULL'
    assert fwd(g=None) == E and fwd(p=None) == E
    assert bwd(go=None) == E and lib.dirt_last_error().decode() == 'dirt_shade_sh_backward: gbuffer / params / grad_out is NULL'
    assert bwd(gc=one) == E
    assert lib.dirt_last_error().decode() == 'dirt_shade_sh_backward: grad_colors without colors (the channel path\'s is part of grad_gbuffer)'
    assert bwd(gg=None, gp=None) == 0      # nothing wanted: nothing is launched
    need = lib.dirt_shade_sh_scratch_bytes(1, 64)
    assert need == 4 * 30 and lib.dirt_shade_sh_scratch_bytes(3, FLAT) == 4 * 30 * 3 * 2
    assert lib.dirt_shade_sh_scratch_bytes(-1, 64) == 0 and lib.dirt_shade_sh_scratch_bytes(65536, 64) == 0 and lib.dirt_shade_sh_scratch_bytes(1, -1) == 0
    assert bwd(nbytes=need - 1) == E
    assert lib.dirt_last_error().decode() == 'dirt_shade_sh_backward: scratch is NULL or smaller than dirt_shade_sh_scratch_bytes (119 < 120)'
    assert bwd(scratch=None) == E and bwd(scratch=ctypes.c_void_p(18)) == E and b'4-byte aligned' in lib.dirt_last_error()


def test_the_kernels_use_no_scratch_memory():
    from dirt_amd import build
    res = {k: v for k, v in build.kernel_resources().items() if 'shade_sh_' in k}
    assert len(res) == 8, sorted(res)       # the forward and <PARAMS, GBUF, TENSOR> without <false, false, false>
    for name, v in res.items():
        assert v['scratch'] == 0 and v['vgpr'] <= 128 and v['lds'] <= 12288, (name, v)


# ---- GPU tests

PATTERNS = [('channel', (True, True, False)), ('channel', (True, False, False)), ('channel', (False, True, False))] + \
           [('tensor', w) for w in ((True, True, True), (True, False, True), (False, True, True), (False, False, True), (True, True, False),
                                    (True, False, False), (False, True, False))]


@pytest.mark.gpu
@pytest.mark.parametrize('path, want', PATTERNS, ids=['%s-%s' % (p, ''.join(n for n, on in zip('gpc', w) if on)) for p, w in PATTERNS])
def test_every_backward_instantiation(gpu, path, want):
    """One flat frame of a workgroup's span + 3 pixels through each pattern of wanted gradients (G-buffer, parameters, colour
    tensor) on both paths; what is not wanted stays None."""
    case, ref, got = compare('pattern_' + path, gpu, want)
    assert ('d_gbuffer' in got) == want[0] and ('d_coefficients' in got) == want[1]
    assert ('d_colors' in got) == (want[2] if path == 'tensor' else want[0])
    compare('outer_' + path, gpu, want)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(_options()))
def test_options_against_the_restatement(gpu, name):
    compare(name, gpu)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(LAYOUTS))
def test_layouts_against_the_restatement(gpu, name):
    compare(name, gpu)


@pytest.mark.gpu
@pytest.mark.parametrize('name', [k for k in CASES if k.startswith('scenes_')])
def test_scenes_that_end_on_and_past_a_workgroup_boundary(gpu, name):
    compare(name, gpu)


@pytest.mark.gpu
def test_strided_colours_are_read_in_place(gpu, monkeypatch):
    """The first and the last three channels of an RGBA image and `gbuffer[..., a:a + 3]`: the pointer the C ABI receives is
    the tensor's own.  A transposed one is copied.  d colours is dense [..., 3] for all of them."""
    from dirt_amd import _stage, _lib
    case, ref = case_of('pattern_tensor')
    seen = []
    call = _stage.call

    def spy(function, dev, *arguments, **kw):
        seen.append((function, arguments))
        return call(function, dev, *arguments, **kw)

    monkeypatch.setattr(_stage, 'call', spy)
    lib = _lib.load()
    for first in (0, 1):
        rgba = torch.full((case.n, 4), 1.e30, device=gpu)
        rgba[:, first:first + 3] = torch.from_numpy(case.colors).to(gpu)
        del seen[:]
        got = shade(case, gpu, colors=rgba[:, first:first + 3])
        (forward,) = [a for f, a in seen if f is lib.dirt_shade_sh_forward]
        (backward,) = [a for f, a in seen if f is lib.dirt_shade_sh_backward]
        assert forward[1] == rgba.data_ptr() + 4 * first and forward[7] == 4 and backward[1] == forward[1] and backward[12] == 4
        check(case, got, ref, 'rgba[..., %d:%d]' % (first, first + 3))
    planes = torch.from_numpy(np.ascontiguousarray(case.colors.T)).to(gpu)
    del seen[:]
    got = shade(case, gpu, colors=planes.t())
    (forward,) = [a for f, a in seen if f is lib.dirt_shade_sh_forward]
    assert forward[7] == 3 and forward[1] != planes.data_ptr()
    check(case, got, ref, 'transposed colours')


@pytest.mark.gpu
def test_channel_path_against_tensor_path_on_the_same_data(gpu, monkeypatch):
    """colors=g[..., 4:7].detach() (read in place, stride 10) against colors=4: pixels, d normals, d mask and the parameter
    gradients have equal bits, and d colours equals channels 4-6 of the channel path's d gbuffer."""
    from dirt_amd import _stage, _lib
    case, ref = case_of('same_data')
    a = shade(case, gpu)
    check(case, a, ref, 'same_data')
    seen = []
    call = _stage.call
    monkeypatch.setattr(_stage, 'call', lambda f, dev, *args, **kw: (seen.append((f, args)), call(f, dev, *args, **kw))[1])
    g = torch.from_numpy(case.g).to(gpu)
    view = g[..., 4:7].detach().requires_grad_(True)
    from dirt_amd import shading
    gl = g.clone().requires_grad_(True)
    L = torch.from_numpy(case.coefficients).to(gpu).requires_grad_(True)
    bg = torch.from_numpy(case.kw['background']).to(gpu).requires_grad_(True)
    out = shading.shade_gbuffer_sh(gl, L, colors=view, normals=7, mask=0, background=bg, clamp=case.kw['clamp'], normalize=True,
                                   band_scale=case.kw['band_scale'])
    out.backward(torch.from_numpy(case.go).to(gpu))
    (forward,) = [args for f, args in seen if f is _lib.load().dirt_shade_sh_forward]
    assert forward[1] == g.data_ptr() + 16 and forward[7] == 10
    assert torch.equal(out.detach(), a['out']) and torch.equal(L.grad, a['d_coefficients']) and torch.equal(bg.grad, a['d_background'])
    assert torch.equal(gl.grad[:, 7:10], a['d_normals']) and torch.equal(gl.grad[:, 0:1], a['d_mask'])
    assert torch.equal(view.grad, a['d_colors']) and not bool(gl.grad[:, 1:7].any())


def _abi(lib, dev, case, n, guard=7):
    """forward and backward through the C ABI on the first n pixels of `case`, every output inside `guard` floats of 12345 on
    both sides -> (out, grad_gbuffer, grad_colors or None, grad_params), the guards checked"""
    from dirt_amd import _lib
    g = torch.from_numpy(case.g[:n]).to(dev).contiguous()
    col = torch.from_numpy(case.colors[:n]).to(dev).contiguous() if case.tensor else None
    block = torch.cat([torch.from_numpy(case.coefficients).reshape(1, 27), torch.from_numpy(case.kw['background']).reshape(1, 3)], 1).to(dev)
    go = torch.from_numpy(case.go[:n]).to(dev).contiguous()

    def guarded(count):
        t = torch.full((count + 2 * guard,), 12345., device=dev)
        return t, t[guard:guard + count]

    bufs = {k: guarded(c) for k, c in (('out', 3 * n), ('gg', case.cg * n), ('gc', 3 * n), ('gp', 30))}
    lo, hi = case.kw['clamp']
    flags = _lib.SHADE_CLAMP | (_lib.SHADE_SH_NORMALIZE if case.kw['normalize'] else 0)
    lay = case.layout
    tail = (1, n, case.cg, 3 if case.tensor else 0, lay.get('colors', -1), lay['normals'], lay['mask'] if lay.get('mask') is not None else -1, 1,
            *case.kw['band_scale'], lo, hi, flags, None)
    cp = col.data_ptr() if case.tensor else None
    nbytes = lib.dirt_shade_sh_scratch_bytes(1, n)
    sfull, scratch = guarded(nbytes // 4)
    torch.cuda.synchronize()
    _lib.check(lib.dirt_shade_sh_forward(g.data_ptr(), cp, block.data_ptr(), bufs['out'][1].data_ptr(), *tail))
    _lib.check(lib.dirt_shade_sh_backward(g.data_ptr(), cp, block.data_ptr(), go.data_ptr(), bufs['gg'][1].data_ptr(),
                                          bufs['gc'][1].data_ptr() if case.tensor else None, bufs['gp'][1].data_ptr(), scratch.data_ptr(), nbytes,
                                          *tail))
    torch.cuda.synchronize()
    for k, (full, inner) in list(bufs.items()) + [('scratch', (sfull, scratch))]:
        if k == 'gc' and not case.tensor:
            assert bool((full == 12345.).all())
            continue
        assert bool((full[:guard] == 12345.).all()) and bool((full[-guard:] == 12345.).all()), k
        assert not bool((inner == 12345.).any()), k
    return bufs['out'][1].reshape(n, 3), bufs['gg'][1].reshape(n, case.cg), bufs['gc'][1].reshape(n, 3) if case.tensor else None, bufs['gp'][1]


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 255, 256, 257, FLAT])
@pytest.mark.parametrize('path', ['channel', 'tensor'])
def test_the_c_abi_writes_inside_its_outputs(gpu, lib, path, n):
    """Guard values around out, grad_gbuffer, grad_colors, grad_params (and the scratch) stay; every element inside is written.
    The results are the wrapper's on the whole frame (which test_every_backward_instantiation holds against the restatement), bit
    for bit: all of them at the whole frame, the first n pixels' at a shorter one (a pass of one pixel, a partial and a full
    pass, a second pass of one pixel), where a pixel's values do not depend on how many follow it."""
    case, ref = case_of('pattern_' + path)
    out, gg, gc, gp = _abi(lib, gpu, case, n)
    got = shade(case, gpu)
    assert torch.equal(out, got['out'][:n]) and torch.equal(gg, got['d_gbuffer'][:n]) and (gc is None or torch.equal(gc, got['d_colors'][:n]))
    if n == case.n:
        assert torch.equal(gp[:27].reshape(9, 3), got['d_coefficients']) and torch.equal(gp[27:], got['d_background'])


def _pixels(dev, rows, L, kw, go=None):
    """hand-made pixels [m, c[3], n[3]] through the fused call and through the float32 and float64 compositions on the same input"""
    from dirt_amd import shading
    layout = dict(mask=0, colors=1, normals=4)
    g = np.asarray(rows, np.float32)
    go = np.ones((len(g), 3), np.float32) if go is None else np.asarray(go, np.float32)
    gt = torch.from_numpy(g).to(dev).requires_grad_(True)
    Lt = torch.from_numpy(np.asarray(L, np.float32)).to(dev).requires_grad_(True)
    bgt = torch.tensor(kw['background'], device=dev, requires_grad=True)
    out = shading.shade_gbuffer_sh(gt, Lt, background=bgt, **layout, **{k: v for k, v in kw.items() if k != 'background'})
    out.backward(torch.from_numpy(go).to(dev))
    got = {'out': out.detach(), 'd_gbuffer': gt.grad, 'd_colors': gt.grad[:, 1:4], 'd_normals': gt.grad[:, 4:7], 'd_mask': gt.grad[:, 0:1],
           'd_coefficients': Lt.grad, 'd_background': bgt.grad}
    refs = [R.compose(g, np.asarray(L, np.float32), layout, grad_out=go, dtype=dt, masses=dt == torch.float64, **kw)
            for dt in (torch.float64, torch.float32)]
    return got, refs[0], refs[1]


def _near(got, r64, r32, keys=('out', 'd_colors', 'd_normals', 'd_mask', 'd_coefficients', 'd_background')):
    """|gpu - f32 composition| and |gpu - ref64| within KERNEL x F32 of the float64 masses, non-finite values in the same places"""
    kind = {'out': 'pixels', 'd_coefficients': 'd_params', 'd_background': 'd_params'}
    mass = {'out': 'mass_out', 'd_colors': 'mass_colors', 'd_normals': 'mass_normals', 'd_mask': 'mass_mask',
            'd_coefficients': 'mass_coefficients', 'd_background': 'mass_background'}
    for k in keys:
        a = got[k].detach().cpu().double().reshape(r64[k].shape)
        for r in (r64[k], r32[k].double()):
            assert torch.equal(torch.isfinite(a), torch.isfinite(r)), k
            ok = torch.isfinite(r)
            bound = KERNEL * F32[kind.get(k, k)] * r64[mass[k]]
            assert bool(((a - r).abs()[ok] <= bound[ok]).all()), (k, a, r, bound)


L_FLAT = [[1., 1., 1.]] + [[0., 0., 0.]] * 8     # E = C0: a flat light, so that a pixel's value is exact


@pytest.mark.gpu
def test_kink_clamp_edges_pass_the_gradient(gpu):
    """Pre-clamp values exactly lo and exactly hi: the edges are put where the kernel's own float32 values land (the least and
    the greatest of an unclamped run, read back), where the gradient passes as without a clamp; one float further in it stops."""
    rows = [[1., 0.5, 0.25, 1., 0., 0., 1.], [1., 1., 0.5, 0.25, 0., 1., 0.]]
    kw = dict(background=(0.2, 0.3, 0.4), clamp=None, normalize=False, band_scale=(1., 1., 1.))
    got, _, _ = _pixels(gpu, rows, L_FLAT, kw)
    lo, hi = float(got['out'].min()), float(got['out'].max())
    assert lo < hi
    edge, r64, r32 = _pixels(gpu, rows, L_FLAT, dict(kw, clamp=(lo, hi)))
    assert torch.equal(edge['out'], got['out'])
    at_lo, at_hi = got['out'] == lo, got['out'] == hi
    assert bool(at_lo.any()) and bool(at_hi.any())
    assert torch.equal(edge['d_colors'][at_lo], got['d_colors'][at_lo]) and torch.equal(edge['d_colors'][at_hi], got['d_colors'][at_hi])
    assert bool((edge['d_colors'][at_lo] != 0).all()) and bool((edge['d_colors'][at_hi] != 0).all())
    inside = ~(at_lo | at_hi)
    assert torch.equal(edge['d_colors'][inside], got['d_colors'][inside])
    # and one step outside the edges the gradient stops
    inner = (float(np.nextafter(np.float32(lo), np.float32(2))), float(np.nextafter(np.float32(hi), np.float32(-2))))
    out2, _, _ = _pixels(gpu, rows, L_FLAT, dict(kw, clamp=inner))
    assert not bool(out2['d_colors'][at_lo].any()) and not bool(out2['d_colors'][at_hi].any())


@pytest.mark.gpu
def test_kink_uncovered_pixels(gpu):
    """m = 0: only the background's and the mask's gradients are non-zero."""
    rng = np.random.default_rng(5500)
    rows = [[0., 0.3, 0.6, 0.9, 0.6, 0., 0.8], [0., 1., 1., 1., 0., 0., 1.]]
    L = R.random_coefficients(rng)
    got, r64, r32 = _pixels(gpu, rows, L, dict(background=(0.2, 0.3, 0.4), clamp=(0., 1.), normalize=False, band_scale=(1., 1., 1.)))
    _near(got, r64, r32)
    assert not bool(got['d_colors'].any()) and not bool(got['d_normals'].any()) and not bool(got['d_coefficients'].any())
    assert bool((got['d_mask'] != 0).all()) and torch.equal(got['d_background'].cpu(), torch.full((3,), 2.))
    assert torch.equal(got['out'].cpu(), torch.tensor([[0.2, 0.3, 0.4]] * 2))


@pytest.mark.gpu
def test_kink_zero_and_tiny_normals_under_normalize(gpu):
    """A zero normal, one shorter than 1e-12 and one of exactly that order with normalize=True: value and gradient are the
    float32 torch composition's on the same input (by the mass rule) -- max(|n|, 1e-12) and the norm's zero gradient at 0."""
    rng = np.random.default_rng(5501)
    rows = [[1., 0.5, 0.6, 0.7, 0., 0., 0.], [1., 0.5, 0.6, 0.7, 3e-13, -4e-13, 0.], [0.5, 0.5, 0.6, 0.7, 6e-12, 0., 8e-12],
            [1., 0.5, 0.6, 0.7, 0.3, -0.4, 1.2]]
    L = R.random_coefficients(rng)
    got, r64, r32 = _pixels(gpu, rows, L, dict(background=(0.2, 0.3, 0.4), clamp=None, normalize=True, band_scale=LAMBERT))
    _near(got, r64, r32)
    assert bool(got['d_normals'][0].abs().max() > 1e9)      # 1 / 1e-12 times the linear terms' gradient
    assert bool(torch.isfinite(got['d_gbuffer']).all())


@pytest.mark.gpu
@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_non_finite_colour_stays_in_its_pixel(gpu, bad):
    case, ref = case_of('pattern_channel')
    clean = shade(case, gpu)
    g = torch.from_numpy(case.g).to(gpu)
    g[300, case.layout['colors'] + 1] = bad
    got = shade(case, gpu, g=g)
    others = torch.ones(case.n, dtype=torch.bool, device=gpu)
    others[300] = False
    assert torch.equal(got['out'][others], clean['out'][others]) and torch.equal(got['d_gbuffer'][others], clean['d_gbuffer'][others])
    if bad != bad:     # a NaN stays a NaN through the clamp; an inf may be clamped
        assert bool(torch.isnan(got['out'][300, 1]))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['c1024', 'scenes_%d_per_scene' % (SPAN + 1)])
def test_two_runs_give_the_same_bits(gpu, name):
    case, _ = case_of(name)
    a, b = shade(case, gpu), shade(case, gpu)
    assert set(a) == set(b)
    for k in a:
        assert a[k] is None and b[k] is None or torch.equal(a[k], b[k]), k


@pytest.mark.gpu
def test_graph_capture_replays_to_the_eager_bits(gpu):
    """Forward and backward captured with torch.cuda.graph (the call makes no host synchronisation) replay to the eager bits."""
    from dirt_amd import shading
    case, _ = case_of('pattern_tensor')
    eager = shade(case, gpu)
    g = torch.from_numpy(case.g).to(gpu).requires_grad_(True)
    col = torch.from_numpy(case.colors).to(gpu).requires_grad_(True)
    L = torch.from_numpy(case.coefficients).to(gpu).requires_grad_(True)
    bg = torch.from_numpy(case.kw['background']).to(gpu).requires_grad_(True)
    go = torch.from_numpy(case.go).to(gpu)

    def step():
        out = shading.shade_gbuffer_sh(g, L, colors=col, normals=case.layout['normals'], mask=case.layout['mask'], background=bg,
                                       clamp=case.kw['clamp'], normalize=case.kw['normalize'], band_scale=case.kw['band_scale'])
        return (out,) + torch.autograd.grad(out, [g, col, L, bg], go)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for t, k in zip(captured, ('out', 'd_gbuffer', 'd_colors', 'd_coefficients', 'd_background')):
        assert torch.equal(t.reshape(eager[k].shape), eager[k]), k


def _load_example(name):
    spec = importlib.util.spec_from_file_location('example_' + name, os.path.join(ROOT, 'examples', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _torch_sh_shader(kw):
    from dirt_amd import lighting

    def shader(gbuffer, table, background):
        m, c, n = gbuffer[..., :1], gbuffer[..., 1:4], gbuffer[..., 4:7]
        lit = lighting.spherical_harmonics(n, c, table, band_scale=kw['band_scale'], normalize=kw['normalize'])
        return torch.clamp(lit * m + background.reshape((-1,) + (1,) * (gbuffer.dim() - 2) + (3,)) * (1. - m), 0., 1.)
    return shader


@pytest.mark.gpu
@pytest.mark.parametrize('batched', [False, True])
def test_rasterise_deferred_with_the_fused_shader(gpu, batched):
    """The example's sphere on a 64 x 48 frame through rasterise_deferred / rasterise_batch_deferred with shade_gbuffer_sh as
    the shader against the same call with the shader written with lighting.spherical_harmonics: pixels, d coefficients and
    d background by the mass rule (masses from the restatement on the rasterised G-buffer).  The vertex gradient comes from
    filtering the shaded image, where a one-ulp pixel difference can flip a discrete choice and no mass is at hand: an
    element agrees if |a - b| <= 1e-3 max(|a|, |b|) (or both are below 1e-7); at most 1 % may not."""
    import dirt_amd
    from dirt_amd import lighting, matrices, shading
    ex = _load_example('fit_sh_lighting_fused')
    W, H = 64, 48
    kw = dict(band_scale=LAMBERT, normalize=True)
    verts_np, faces_np, cols_np = ex.build_sphere()
    B = 2 if batched else 1
    tables = torch.stack([ex.true_coefficients(gpu) / math.pi * (1. + 0.3 * b) for b in range(B)])
    grounds = torch.tensor([[0.1, 0.1, 0.2], [0.3, 0.2, 0.1]], device=gpu)[:B]
    results = []
    for fused in (False, True):
        vertices = torch.from_numpy(verts_np).to(gpu).requires_grad_(True)
        faces, colors = torch.from_numpy(faces_np).to(gpu), torch.from_numpy(cols_np).to(gpu)
        table = (tables if batched else tables[0]).clone().requires_grad_(True)
        ground = (grounds if batched else grounds[0]).clone().requires_grad_(True)
        view = matrices.translation(torch.tensor([0., 0., -3.], device=gpu))
        projection = matrices.perspective_projection(near=0.1, far=20., right=0.05, aspect=float(H) / W).to(gpu)
        clip = (torch.cat([vertices, torch.ones_like(vertices[:, :1])], 1) @ view) @ projection
        attributes = torch.cat([torch.ones_like(vertices[:, :1]), colors, 1.7 * lighting.vertex_normals(vertices, faces)], 1)
        if fused:
            def fn(gbuffer, t, b):
                return shading.shade_gbuffer_sh(gbuffer, t, background=b, **ex.LAYOUT, **kw)
        else:
            fn = _torch_sh_shader(kw)
        if batched:
            pixels = dirt_amd.rasterise_batch_deferred(torch.zeros([B, H, W, 7], device=gpu), clip[None].repeat(B, 1, 1),
                                                       attributes[None].repeat(B, 1, 1), faces[None].repeat(B, 1, 1), fn, [table, ground])
            gbuf = dirt_amd.rasterise_batch(torch.zeros([B, H, W, 7], device=gpu), clip.detach()[None].repeat(B, 1, 1),
                                            attributes.detach()[None].repeat(B, 1, 1), faces[None].repeat(B, 1, 1))
        else:
            pixels = dirt_amd.rasterise_deferred(torch.zeros([H, W, 7], device=gpu), clip, attributes, faces, fn, [table, ground])
            gbuf = dirt_amd.rasterise(torch.zeros([H, W, 7], device=gpu), clip.detach(), attributes.detach(), faces)
        (pixels ** 2).mean().backward()
        results.append((pixels.detach(), vertices.grad, table.grad, ground.grad, gbuf))
    (pa, va, ta, ga, gbuf), (pb, vb, tb, gb, _) = results
    go = (2. / pa.numel()) * pa.reshape(-1, 3).cpu().numpy()
    idx = np.repeat(np.arange(B), H * W) if batched else None
    ref = R.compose(gbuf.reshape(-1, 7).cpu().numpy(), tables.cpu().numpy() if batched else tables[0].cpu().numpy(), ex.LAYOUT,
                    background=grounds.cpu().numpy() if batched else grounds[0].cpu().numpy(), grad_out=go, scene_index=idx, **kw)
    assert 0.2 < float((gbuf[..., 0] > 0).float().mean()) < 0.8
    for what, a, b, mass, f in (('pixels', pa, pb, ref['mass_out'], F32['pixels']), ('d_coefficients', ta, tb, ref['mass_coefficients'], F32['d_params']),
                                ('d_background', ga, gb, ref['mass_background'], F32['d_params'])):
        a, b = a.cpu().double().reshape(mass.shape), b.cpu().double().reshape(mass.shape)
        r = ref['out' if what == 'pixels' else what]
        for x, y, factor in ((b, r, KERNEL), (b, a, KERNEL + 1)):     # against the restatement; against the torch shader, which has its own F32
            assert bool(((x - y).abs() <= factor * f * mass).all()), (what, float(((x - y).abs() / mass.clamp_min(1e-300)).max()), f)
    a, b = va.cpu().double(), vb.cpu().double()
    agree = ((a - b).abs() <= 1e-3 * torch.maximum(a.abs(), b.abs())) | ((a.abs() < 1e-7) & (b.abs() < 1e-7))
    print('deferred: d_vertices: %d of %d elements excluded' % (int((~agree).sum()), agree.numel()))
    assert 1. - float(agree.double().mean()) <= 0.01 and bool(a.abs().max() > 0)


@pytest.mark.gpu
def test_the_example_recovers_the_light(gpu):
    ex = _load_example('fit_sh_lighting_fused')
    losses, before, after = ex.fit(width=64, height=48, steps=30, device=gpu)
    assert losses[-1] < losses[0] and after < before


def _many(dev):
    """-> (run, pixels, grad_out, values) of `pattern_channel` for the many-scenes checks of tests/test_shade.py"""
    from dirt_amd import shading
    case, _ = case_of('pattern_channel')
    values = {'coefficients': torch.from_numpy(case.coefficients).to(dev), 'background': torch.from_numpy(case.kw['background']).to(dev)}

    def run(g, values, go):
        g = g.detach().requires_grad_(True)
        named = {k: v.detach().requires_grad_(True) for k, v in values.items()}
        out = shading.shade_gbuffer_sh(g, named['coefficients'], colors=case.layout['colors'], normals=case.layout['normals'],
                                       mask=case.layout['mask'], background=named['background'], clamp=case.kw['clamp'],
                                       normalize=case.kw['normalize'], band_scale=case.kw['band_scale'])
        out.backward(go)
        return out.detach(), g.grad, {k: t.grad for k, t in named.items()}

    return run, case.g, case.go, values


@pytest.mark.gpu
def test_65535_scenes_of_one_pixel(gpu):
    """the grid's y dimension at its limit and 65535 rows in shade_launch_reduce: tests/test_shade.py::many_scenes"""
    from tests import test_shade
    run, pixels, _, values = _many(gpu)
    assert SPAN == test_shade.SPAN
    test_shade.many_scenes(run, gpu, pixels, values, 5400, 'shade_gbuffer_sh')


@pytest.mark.gpu
def test_a_2x512x512_frame_adds_512_rows(gpu):
    """512 rows of partial sums shared by two scenes: tests/test_shade.py::frame_of_512_rows"""
    from tests import test_shade
    run, pixels, grad_out, values = _many(gpu)
    test_shade.frame_of_512_rows(run, gpu, pixels[:SPAN], grad_out[:SPAN], values, 5401, 'shade_gbuffer_sh')
