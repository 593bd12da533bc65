"""`shade_gbuffer_pbr` (dirt_shade_pbr.hip) where tests/test_shade_pbr.py does not reach: the nine backward instantiations
<0 | 1 | 4 lights, PARAMS, GBUF> no test there launches, the kinks the older shaders pin (an uncovered pixel, the clamp's
edges) and two of its own (a light shining straight at the camera, a point light at the pixel), non-finite values staying in
their pixel, 65535 scenes and more than 256 rows of partial sums in `block_column_sum`, an expanded and a strided grad_out,
and the C ABI with `grad_params` alone.  Cases, references, bounds and helpers are those of tests/test_shade_pbr.py.

The many-scenes checks and the derived bound of the reduce are those of tests/test_shade.py (`many_scenes`, `frame_of_512_rows`,
`within_the_reduce_bound`), which the three shaders share as they share `shade_launch_reduce`.
"""
import copy

import numpy as np
import pytest
import torch

from tests import shade_pbr_reference as R
from tests import test_shade as S
from tests import test_shade_pbr as T

D, P = T.D, T.P


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import _lib, build
    build.build_library()
    return _lib.load()


def _launches(monkeypatch):
    """-> list that receives (entry point, arguments) of every call into the C ABI from here on"""
    from dirt_amd import _stage
    seen, call = [], _stage.call
    monkeypatch.setattr(_stage, 'call', lambda f, dev, *args, **kw: (seen.append((f, args)), call(f, dev, *args, **kw))[1])
    return seen


def _same_bits(got, full, what):
    """every result of `got` has the bits it has in `full`, the run of the same inputs with every gradient wanted"""
    for k, v in got.items():
        if k == 'd_params':
            for name, x in v.items():
                assert torch.equal(x, full['d_params'][name]), (what, name)
        else:
            assert torch.equal(v, full[k]), (what, k)


# ---- A. every backward instantiation no test of tests/test_shade_pbr.py launches

PARAMS_ONLY, GBUFFER_ONLY = (False, True, False, False), (True, False, False, False)
BOTH_TENSORS, COLORS_ONLY, MATERIAL_ONLY = (False, False, True, True), (False, False, True, False), (False, False, False, True)
REACH = [   # case, wanted gradients of (G-buffer, parameters, colour tensor, material tensor), the instantiation <lights, PARAMS, GBUF>
    ('lights_0', PARAMS_ONLY, (0, True, False)), ('lights_0', GBUFFER_ONLY, (0, False, True)), ('pattern_tensors_0', BOTH_TENSORS, (0, False, False)),
    ('lights_1_point', PARAMS_ONLY, (1, True, False)), ('lights_1_point', GBUFFER_ONLY, (1, False, True)),
    ('tensors-mask-narrow', BOTH_TENSORS, (1, False, False)),
    ('lights_4_mixed', PARAMS_ONLY, (4, True, False)), ('lights_4_mixed', GBUFFER_ONLY, (4, False, True)),
    ('tensors-mask-noclamp', BOTH_TENSORS, (4, False, False)), ('tensors-mask-noclamp', COLORS_ONLY, (4, False, False)),
    ('tensors-mask-noclamp', MATERIAL_ONLY, (4, False, False)),
]


@pytest.mark.gpu
@pytest.mark.parametrize('name, want, kernel', REACH,
                         ids=['%d%s%s-%s-%s' % (k[0], 'TF'[not k[1]], 'TF'[not k[2]], n, ''.join(c for c, on in zip('gpcm', w) if on)) for n, w, k in REACH])
def test_every_backward_instantiation(gpu, monkeypatch, name, want, kernel):
    """The one backward launch is the instantiation named (read off the arguments the C ABI receives: the light count, whether
    grad_params and grad_gbuffer are there); what is wanted agrees with the restatement by the mass rule and has the bits of
    the run with every gradient wanted -- a pixel's arithmetic does not depend on the instantiation, and the parameter sums
    are added in a fixed order; what is not wanted is absent, a NULL pointer at the C ABI."""
    from dirt_amd import _lib
    seen = _launches(monkeypatch)
    case, ref, got = T.compare(name, gpu, want)
    (args,) = [a for f, a in seen if f is _lib.load().dirt_shade_pbr_backward]
    assert (args[22], args[8] is not None, args[5] is not None) == kernel, (args[22], args[8], args[5])
    assert (args[6] is not None, args[7] is not None) == want[2:]
    assert len(case.kinds) == kernel[0]
    expected = {'out'} | ({'d_gbuffer'} | {'d_' + k for k, _ in R.ATTRIBUTES if case.layout.get(k) is not None} if want[0] else set()) | \
        ({'d_params'} if want[1] else set()) | ({'d_colors'} if want[2] else set()) | ({'d_material'} if want[3] else set())
    assert set(got) == expected
    _same_bits(got, T.shade(case, gpu), name)


# ---- B. kinks: hand-made pixels [m, c[3], n[3], p[3], r, mu] of KINK_LAYOUT

FACING = [0.5, 0.25, 0.75, 0.25, 0.25, 1., 0.25, -0.5, 0.5, 0.5, 0.5]      # a pixel seen along -z from KINK_KW's camera: v = (0, 0, 1)


@pytest.mark.gpu
def test_kink_an_uncovered_pixel_with_a_unit_normal(gpu):
    """m = 0 beside the same pixel covered: the output is the background exactly, colours, normal, position and material get
    exact zeros, the mask gets sum_j go_j (lit_j - background_j); alone, the pixel leaves d background = go and every other
    parameter gradient an exact zero."""
    row = [0.5, 0.25, 0.75, 0., 0., 1., 0.25, -0.5, 0.5, 0.5, 0.5]
    got, r64, r32 = T._pixels(gpu, [[0.] + row, [1.] + row])
    T._near(got, r64, r32)
    background = torch.tensor(T.KINK_KW['background'], device=gpu)
    assert torch.equal(got['out'][0], background)
    for k in ('colors', 'normals', 'positions', 'material'):
        assert bool((got['d_' + k][0] == 0).all()), k
    lit = r64['out'][1]      # the covered twin, no clamp: its output is the lit colour
    want = float((lit - torch.tensor(T.KINK_KW['background'], dtype=torch.float32).double()).sum())
    assert abs(float(r64['d_mask'][0, 0]) - want) <= 1e-14 and abs(want) > 0.1
    alone, a64, a32 = T._pixels(gpu, [[0.] + row])
    T._near(alone, a64, a32)
    for k, v in alone['d_params'].items():
        assert torch.equal(v, torch.ones(3, device=gpu)) if k == 'background' else bool((v == 0).all()), (k, v)


@pytest.mark.gpu
def test_kink_clamp_edges_pass_the_gradient(gpu):
    """Without lights, ambient 0.5 and clamp (0.25, 1): the pre-clamp values are colour / 2, exactly at lo, at hi, above and
    below; torch's clamp passes the gradient at both edges and stops it outside."""
    kw = dict(T.KINK_KW, ambient=(0.5, 0.5, 0.5), clamp=(0.25, 1.))
    tail = [0.25, 0.25, 1., 0.25, -0.5, 0.5, 0.5, 0.5]
    rows = [[1., 0.5, 2., 2.5] + tail,      # pre = 0.25 (lo), 1 (hi), 1.25 (above)
            [1., 0.25, 1., 0.5] + tail]     # pre = 0.125 (below), 0.5, 0.25 (lo)
    got, r64, r32 = T._pixels(gpu, rows, lights=[], kw=kw)
    assert r64['pre'].tolist() == [[0.25, 1., 1.25], [0.125, 0.5, 0.25]]
    T._near(got, r64, r32)
    assert got['out'].tolist() == [[0.25, 1., 1.], [0.25, 0.5, 0.25]]
    assert got['d_colors'][0].tolist() == [0.5, 0.5, 0.] and got['d_colors'][1].tolist() == [0., 0.5, 0.5]
    assert got['d_params']['ambient'].tolist() == [0.5, 3., 0.5]      # sum of the colours where the gate is open


@pytest.mark.gpu
def test_kink_a_light_shining_straight_at_the_camera(gpu):
    """v = (0, 0, 1) exactly and a directional light along +z: l + v = 0, h = 0, den = 0 and D = a2 / 0.  Output and d gbuffer
    have their non-finite values in the places of the float32 composition; the pixel beside it has the bits it has alone."""
    lights = [(D, (0., 0., 1.), (0.5, 0.5, 0.5)), T.KINK_LIGHTS[1]]
    rows = [[1.] + FACING, [1., 0.5, 0.25, 0.75, 0.25, 0.25, 1., 0.5, -0.25, 0.25, 0.5, 0.5]]
    got, r64, r32 = T._pixels(gpu, rows, lights=lights)
    alone, _, _ = T._pixels(gpu, rows[1:], lights=lights)
    assert r64['cosines'][0, 1:4].tolist() == [-r64['cosines'][0, 0].item(), 0., 0.]     # n . l = -n . v; n . h = v . h = 0: h is the zero vector
    for k in ('out', 'd_gbuffer'):
        assert torch.equal(torch.isfinite(got[k]).cpu(), torch.isfinite(r32[k])), (k, got[k], r32[k])
        assert torch.equal(got[k][1], alone[k][0]), k
    assert not bool(torch.isfinite(got['out'][0]).any()) and bool(torch.isfinite(got['d_gbuffer'][1]).all())


@pytest.mark.gpu
def test_kink_a_point_light_at_the_pixel(gpu):
    """p equal to the point light's position: l = 0 / max(0, 1e-12) = 0, h = v, n . l = 0 at its kink, everything finite and
    the norm's gradient 0.  Then the light 1e-13 from a pixel at the origin: |d - p| lies under the 1e-12 of the
    normalisation, l = (d - p) 1e12 is a tenth of a unit vector, and max(|x|, 1e-12) passes nothing to |x|."""
    rows = [[1., 0.5, 0.25, 0.75, 0., -1., 0.5, 1., 2., 3., 0.5, 0.5]]
    got, r64, r32 = T._pixels(gpu, rows)
    assert r64['cosines'][0, 4].item() == 0. and r64['cosines'][0, 0].item() > 0.5
    T._near(got, r64, r32)
    assert bool(torch.isfinite(got['d_gbuffer']).all()) and all(bool(torch.isfinite(v).all()) for v in got['d_params'].values())
    lights = [T.KINK_LIGHTS[0], (P, (1.e-13, 0., 0.), (0.25, 0.5, 0.5))]
    rows = [[1., 0.5, 0.25, 0.75, 0.5, 0.25, 1., 0., 0., 0., 0.5, 0.5]]
    got, r64, r32 = T._pixels(gpu, rows, lights=lights)
    assert 0.04 < r64['cosines'][0, 4].item() < 0.05      # n . l with |l| = 0.1
    T._near(got, r64, r32)
    assert bool(torch.isfinite(got['d_gbuffer']).all()) and float(got['d_params']['light1.vector'].abs().max()) > 1e9


# ---- C. non-finite values stay in their pixel

ATTRIBUTES = {'colors': ('colors', 0), 'roughness': ('material', 0), 'metalness': ('material', 1), 'normals': ('normals', 0),
              'positions': ('positions', 0), 'mask': ('mask', 0)}
_CLEAN = {}


def _clean(name, clamp, dev):
    """-> (a copy of case `name` under `clamp`, its fused run, the victim: a fully covered pixel), made once"""
    if (name, clamp) not in _CLEAN:
        case = T.case_of(name)[0] if clamp == T.CASES[name].get('clamp', (0., 1.)) else T.Case(**dict(T.CASES[name], clamp=clamp))
        victim = 137 + int(np.argmax(case.g[137:, case.layout['mask']] == 1.))
        _CLEAN[name, clamp] = (case, T.shade(case, dev), victim)
    return _CLEAN[name, clamp]


@pytest.mark.gpu
@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
@pytest.mark.parametrize('attribute', list(ATTRIBUTES))
@pytest.mark.parametrize('clamp', [None, (0., 1.)], ids=['noclamp', 'clamp'])
@pytest.mark.parametrize('name', ['pattern_channels', 'pattern_tensors'])
def test_non_finite_values_stay_in_their_pixel(gpu, name, clamp, attribute, bad):
    """One attribute of one covered pixel made NaN, then +inf.  Every other pixel's output and gradients keep the bits of the
    run on the clean data.  The victim's output is non-finite exactly where the float64 restatement's (of that pixel alone)
    is; its gradients and the parameter gradients are non-finite at least wherever the restatement's are -- no silently
    finite value.  (Where only the kernel is non-finite is printed: DESIGN.md §7b lists the places.)"""
    clean_case, clean, victim = _clean(name, clamp, gpu)
    case = copy.copy(clean_case)
    case.g, case.colors, case.material = (None if x is None else x.copy() for x in (clean_case.g, clean_case.colors, clean_case.material))
    key, channel = ATTRIBUTES[attribute]
    if key in case.layout:
        case.g[victim, case.layout[key] + channel] = bad
    else:
        getattr(case, key)[victim, channel] = bad
    got = T.shade(case, gpu)
    one = lambda x: None if x is None else x[victim:victim + 1]   # noqa: E731
    ref = R.compose(one(case.g), case.lights, case.layout, colors=one(case.colors), material=one(case.material), grad_out=one(case.go),
                    masses=False, **case.kw)
    others = torch.arange(case.n, device=gpu) != victim
    kinds = [k for k in ('out', 'd_gbuffer', 'd_colors', 'd_material') if k in got]
    assert 'd_gbuffer' in kinds and 'd_colors' in kinds and 'd_material' in kinds
    for k in kinds:
        assert torch.equal(got[k][others], clean[k][others]), k
    fin = lambda x: torch.isfinite(x.detach().cpu()).reshape(-1)   # noqa: E731
    assert torch.equal(fin(got['out'][victim]), fin(ref['out'][0])), (got['out'][victim], ref['out'][0])
    wider = []
    for k in kinds[1:] + list(got['d_params']):
        a, r = (got[k][victim], ref[k][0]) if k in kinds else (got['d_params'][k], ref['d_params'][k])
        silent = fin(a) & ~fin(r)
        assert not bool(silent.any()), '%s: finite where the restatement is not: %s against %s' % (k, a, r)
        if bool((~fin(a) & fin(r)).any()):
            wider.append(k)
    print('non-finite in the kernel alone (%s %s %s %s): %s' % (name, 'clamp' if clamp else 'noclamp', attribute, bad, ', '.join(wider) or 'nowhere'))


# ---- D. many scenes, many rows of partial sums

def _run(dev, g, prm, kinds, go):
    """`shade_gbuffer_pbr` on a c12 G-buffer (GPU tensor [..., 12]) with the parameters `prm` {name: GPU tensor}, backward with
    `go` as it is handed over -> (out, d gbuffer, {name: gradient})"""
    from dirt_amd import shading
    lay = T.LAYOUTS['c12'][1]
    g = g.detach().requires_grad_(True)
    prm = {k: v.detach().requires_grad_(True) for k, v in prm.items()}
    lights = [(kind, prm['light%d.vector' % i], prm['light%d.color' % i]) for i, kind in enumerate(kinds)]
    out = shading.shade_gbuffer_pbr(g, lights, ambient=prm['ambient'], camera_position=prm['camera_position'], background=prm['background'], **lay)
    out.backward(go)
    return out.detach(), g.grad, {k: v.grad for k, v in prm.items()}


@pytest.mark.gpu
def test_65535_scenes_of_one_pixel(gpu):
    """the grid's y dimension at its limit, a block per scene and one block for 65535 rows, with two lights:
    tests/test_shade.py::many_scenes"""
    case, _ = T.case_of('pattern_channels')
    assert T.SPAN == S.SPAN and len(case.kinds) == 2
    S.many_scenes(lambda g, prm, go: _run(gpu, g, prm, case.kinds, go), gpu, case.g, {k: torch.from_numpy(v).to(gpu) for k, v in case.params.items()},
                  6500, 'shade_gbuffer_pbr')


@pytest.mark.gpu
def test_a_2x512x512_frame_adds_512_rows(gpu):
    """512 rows of partial sums shared by two scenes, whole workgroups in the reduce loop's second turn:
    tests/test_shade.py::frame_of_512_rows on the first workgroup's span of `pattern_channels`"""
    case, _ = T.case_of('pattern_channels')
    S.frame_of_512_rows(lambda g, prm, go: _run(gpu, g, prm, case.kinds, go), gpu, case.g[:T.SPAN], case.go[:T.SPAN],
                        {k: torch.from_numpy(v).to(gpu) for k, v in case.params.items()}, 6501, 'shade_gbuffer_pbr')


# ---- E. grad_out as autograd hands it over; the C ABI with grad_params alone

@pytest.mark.gpu
def test_an_expanded_and_a_strided_grad_out(gpu):
    """`out.mean().backward()` hands backward an expanded grad_out (stride 0): the bits of the dense constant.  A slice
    `[..., :3]` of a four-channel image as grad_out: the bits of the run on its dense copy."""
    case, _ = T.case_of('pattern_channels')
    g = torch.from_numpy(case.g).to(gpu).reshape(13, 79, case.cg)
    prm = {k: torch.from_numpy(v).to(gpu) for k, v in case.params.items()}

    def run(go):
        return _run(gpu, g, prm, case.kinds, go)

    def mean():
        from dirt_amd import shading
        leaf, p = g.detach().requires_grad_(True), {k: v.detach().requires_grad_(True) for k, v in prm.items()}
        lights = [(kind, p['light%d.vector' % i], p['light%d.color' % i]) for i, kind in enumerate(case.kinds)]
        out = shading.shade_gbuffer_pbr(leaf, lights, ambient=p['ambient'], camera_position=p['camera_position'], background=p['background'],
                                        **T.LAYOUTS['c12'][1])
        out.mean().backward()
        return out.detach(), leaf.grad, {k: v.grad for k, v in p.items()}

    constant = torch.full((13, 79, 3), 1. / (13 * 79 * 3), device=gpu)
    expanded = torch.tensor(1. / (13 * 79 * 3), device=gpu).expand(13, 79, 3)
    image = torch.from_numpy(np.random.default_rng(6502).standard_normal((13, 79, 4)).astype(np.float32)).to(gpu)
    assert expanded.stride() == (0, 0, 0) and not image[..., :3].is_contiguous()
    for what, a, b in (('mean', mean(), run(constant)), ('expanded', run(expanded), run(constant)),
                       ('slice', run(image[..., :3]), run(image[..., :3].contiguous()))):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool(a[1].any()), what
        for k in a[2]:
            assert torch.equal(a[2][k], b[2][k]), (what, k)


@pytest.mark.gpu
def test_the_c_abi_with_grad_params_alone_and_a_block_per_scene(gpu, lib):
    """param_scenes = scenes = 3, every gradient pointer but grad_params NULL, the scratch of dirt_shade_pbr_scratch_bytes:
    the wrapper's bits, and the guard floats around grad_params and the scratch intact."""
    from dirt_amd import _lib
    case, _ = T.case_of('scenes_%d_per_scene' % (T.SPAN + 1))
    scenes, pixels, nl, guard = 3, T.SPAN + 1, len(case.kinds), 7
    width = 9 + 8 * nl
    block = np.zeros((scenes, width), np.float32)
    block[:, 0:3], block[:, 3:6], block[:, 6:9] = case.params['ambient'], case.params['background'], case.params['camera_position']
    for i in range(nl):
        block[:, 9 + 8 * i:12 + 8 * i], block[:, 12 + 8 * i:15 + 8 * i] = case.params['light%d.vector' % i], case.params['light%d.color' % i]
    g, col, mat, go, block = (torch.from_numpy(x).to(gpu).contiguous() for x in (case.g, case.colors, case.material, case.go, block))
    nbytes = lib.dirt_shade_pbr_scratch_bytes(scenes, pixels, nl)
    assert nbytes == 4 * width * scenes * 2
    gp_full, sc_full = (torch.full((count + 2 * guard,), 12345., device=gpu) for count in (scenes * width, nbytes // 4))
    gp, scratch = gp_full[guard:-guard], sc_full[guard:-guard]
    lay = case.layout
    kinds = sum(1 << i for i, kind in enumerate(case.kinds) if kind == P)
    torch.cuda.synchronize()
    _lib.check(lib.dirt_shade_pbr_backward(g.data_ptr(), col.data_ptr(), mat.data_ptr(), block.data_ptr(), go.data_ptr(), None, None, None,
                                           gp.data_ptr(), scratch.data_ptr(), nbytes, scenes, pixels, case.cg, 3, 2, -1, -1, lay['normals'],
                                           lay['positions'], lay['mask'], scenes, nl, kinds, case.kw['min_roughness'], case.kw['dielectric_f0'],
                                           *case.kw['clamp'], _lib.SHADE_CLAMP, None))
    torch.cuda.synchronize()
    for full, inner in ((gp_full, gp), (sc_full, scratch)):
        assert bool((full[:guard] == 12345.).all()) and bool((full[-guard:] == 12345.).all()) and not bool((inner == 12345.).any())
    want = T.shade(case, gpu, PARAMS_ONLY)['d_params']
    gp = gp.reshape(scenes, width)
    for k, lo in [('ambient', 0), ('background', 3), ('camera_position', 6)] + [('light%d.%s' % (i, f), 9 + 8 * i + o) for i in range(nl)
                                                                                  for f, o in (('vector', 0), ('color', 3))]:
        assert torch.equal(gp[:, lo:lo + 3], want[k]), k
    for i in range(nl):
        assert not bool(gp[:, 15 + 8 * i:17 + 8 * i].any())
