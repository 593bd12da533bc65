"""What `shading.resolve_image` and its torch form `lighting.resolve_image` owe without a GPU: the wrapper's refusals in full, the
C ABI's declarations, the float32 torch form against the float64 restatement (the F32 table of tests/test_resolve.py), its
gradients at the kinks, the sRGB pair, and the conditions the test inputs must keep."""
import os
import re

import numpy as np
import pytest
import torch

from tests import resolve_reference as R
from tests.test_resolve import F32, SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IMAGE = torch.zeros(4, 6, 3)
BATCH = torch.zeros(2, 4, 6, 3)

REFUSALS = [
    (dict(image=[1, 2]), 'resolve_image expects image [S H, S W, C] or [B, S H, S W, C], got ()'),
    (dict(image=torch.zeros(4, 6)), 'resolve_image expects image [S H, S W, C] or [B, S H, S W, C], got (4, 6)'),
    (dict(image=torch.zeros(4, 6, 5)), 'resolve_image: image has 5 channels, 1..4'),
    (dict(image=torch.zeros(4, 6, 0)), 'resolve_image: image has 0 channels, 1..4'),
    (dict(image=IMAGE.double()), 'image must be float32, got torch.float64'),
    (dict(factor=0), 'resolve_image: factor must be an int in 1..4, got 0'),
    (dict(factor=5), 'resolve_image: factor must be an int in 1..4, got 5'),
    (dict(factor=2.), 'resolve_image: factor must be an int in 1..4, got 2.0'),
    (dict(factor=True), 'resolve_image: factor must be an int in 1..4, got True'),
    (dict(factor=4), 'resolve_image: an image of 4 x 6 samples is no multiple of factor=4 each way'),
    (dict(factor=3), 'resolve_image: an image of 4 x 6 samples is no multiple of factor=3 each way'),
    (dict(add=torch.zeros(4, 6, 4)), 'resolve_image: add must have the shape of image, (4, 6, 3), got (4, 6, 4)'),
    (dict(add=BATCH), 'resolve_image: add must have the shape of image, (4, 6, 3), got (2, 4, 6, 3)'),
    (dict(add=3.), 'resolve_image: add must have the shape of image, (4, 6, 3), got ()'),
    (dict(add=IMAGE.double()), 'add must be float32, got torch.float64'),
    (dict(add=IMAGE.to('meta')), 'add is on meta, the image on cpu'),
    (dict(curve='filmic'), "resolve_image: curve must be 'linear', 'reinhard' or 'aces', got 'filmic'"),
    (dict(encode='gamma'), "resolve_image: encode must be 'linear' or 'srgb', got 'gamma'"),
    (dict(curve='reinhard'), "resolve_image: white goes with curve='reinhard' and only with it (got curve='reinhard', white=None)"),
    (dict(curve='aces', white=2.), "resolve_image: white goes with curve='reinhard' and only with it (got curve='aces', white=2.0)"),
    (dict(curve='reinhard', white=0.), 'resolve_image: white must be a positive number or a tensor, got 0.0'),
    (dict(curve='reinhard', white='x'), "resolve_image: white must be a positive number or a tensor, got 'x'"),
    (dict(curve='reinhard', white=torch.ones(2, 1)), 'white must have shape [] or [B], got (2, 1)'),
    (dict(curve='reinhard', white=torch.ones(2).double()), 'white must be float32, got torch.float64'),
    (dict(curve='reinhard', white=torch.ones(()).to('meta')), 'white is on meta, the image on cpu'),
    (dict(exposure=(1., 2.)), 'exposure must be 3 numbers, got 2'),
    (dict(exposure='abc'), "exposure must be 3 numbers or a tensor, got 'abc'"),
    (dict(exposure=torch.ones(2, 2)), 'exposure must have shape [3] or [B, 3], got (2, 2)'),
    (dict(exposure=torch.ones(3).double()), 'exposure must be float32, got torch.float64'),
    (dict(exposure=torch.ones(3).to('meta')), 'exposure is on meta, the image on cpu'),
    (dict(clamp=(1., 0.)), 'clamp needs lo <= hi, got (1.0, 0.0)'),
    (dict(clamp=3.), 'clamp must be (lo, hi) or None, got 3.0'),
    (dict(image=BATCH, exposure=torch.ones(3, 3)), 'resolve_image: 2 scenes of image, 3 of exposure'),
    (dict(exposure=torch.ones(3, 3), curve='reinhard', white=torch.ones(2)), 'resolve_image: 3 scenes of exposure, 2 of white'),
]


@pytest.mark.parametrize('change, text', REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_python_refusals_in_full(change, text):
    """Every ValueError of the wrapper with its full text, on types, shapes and devices alone: on a machine without a GPU"""
    from dirt_amd import shading
    kw = dict(dict(image=IMAGE, factor=2), **change)
    image = kw.pop('image')
    with pytest.raises(ValueError) as info:
        shading.resolve_image(image, **kw)
    assert str(info.value) == text


def test_a_cpu_tensor_is_a_runtime_error():
    from dirt_amd import shading
    with pytest.raises(RuntimeError) as info:
        shading.resolve_image(IMAGE, add=IMAGE, factor=2, exposure=torch.ones(3), curve='reinhard', white=torch.ones(()), encode='srgb')
    assert str(info.value) == 'dirt_amd.shading.resolve_image runs on an MI355X only; there is no CPU fallback'


def test_the_header_and_the_binding_declare_the_entry_points():
    from dirt_amd import _lib, build, lighting
    header = open(os.path.join(ROOT, 'include', 'dirt_hip.h')).read()
    for name in ('dirt_resolve_forward', 'dirt_resolve_backward', 'dirt_resolve_scratch_bytes'):
        assert re.search(r'\b(int|size_t) %s\(' % name, header), name
        assert name in _lib.SYMBOLS
    defines = dict(re.findall(r'#define (DIRT_RESOLVE_\w+) (\d+)u?', header))
    assert int(defines['DIRT_RESOLVE_MAX_FACTOR']) == _lib.RESOLVE_MAX_FACTOR == lighting.RESOLVE_MAX_FACTOR == 4
    assert int(defines['DIRT_RESOLVE_MAX_CHANNELS']) == _lib.RESOLVE_MAX_CHANNELS == lighting.RESOLVE_MAX_CHANNELS == 4
    assert {k: int(defines['DIRT_RESOLVE_' + k.upper()]) for k in lighting.RESOLVE_CURVES} == _lib.RESOLVE_CURVES
    assert {k: int(defines['DIRT_RESOLVE_ENCODE_' + k.upper()]) for k in lighting.RESOLVE_ENCODINGS} == _lib.RESOLVE_ENCODINGS
    assert int(defines['DIRT_RESOLVE_CLAMP']) == _lib.RESOLVE_CLAMP
    assert 'dirt_resolve.hip' in build.SOURCES
    assert _lib.ABI_VERSION == 4 and re.search(r'#define DIRT_ABI_VERSION 4\b', header)


@pytest.mark.parametrize('name', R.NAMES)
def test_the_float32_torch_form_against_the_restatement(name):
    """Per element, relative to the element's mass: within the F32 table, whose figures are this test's own worst ones"""
    c = R.case(name)
    got = R.torch_form(c.image, c.add, c.go, **c.kw)
    worst = R.ratios(got, c.ref)
    print(name, {k: '%.2e' % v for k, v in worst.items()})
    for kind, x in worst.items():
        assert got[kind].shape == np.shape(c.ref[kind]), kind
        assert x <= F32[kind], (kind, x)
    assert R.exact_where_massless(got, c.ref)


def test_the_table_is_the_measured_one():
    """`python -m tests.resolve_reference` reproduces the F32 table to within 10 %"""
    for kind, x in R.measure_f32().items():
        assert 0.9 * F32[kind] <= x <= F32[kind], (kind, x)


def test_the_float64_torch_form_is_the_restatement():
    """In float64 the two are the same function: 1e-12 of the mass, values and gradients"""
    for name in ('grid-2-aces-srgb', 'grid-3-reinhard-srgb', 'batch-111', 'batch-010', 'clamp-inner-reinhard', 'channels-4-3'):
        c = R.case(name)
        got = R.torch_form(c.image, c.add, c.go, dtype=torch.float64, **c.kw)
        for kind, x in R.ratios(got, c.ref).items():
            assert x <= 1e-12, (name, kind, x)


@pytest.mark.parametrize('curve', R.CURVES)
def test_the_torch_form_has_finite_gradients_at_the_floor_and_at_the_knee(curve):
    """u = 0 and u = knee exactly: the power's branch is not taken, and puts no inf * 0 into the gradient"""
    from dirt_amd import lighting
    x = torch.tensor([[[0., lighting.SRGB_KNEE, -1., 1e-30]]], requires_grad=True)
    white = 2. if curve == 'reinhard' else None
    y = lighting.resolve_image(x, curve=curve, white=white, encode='srgb')
    y.sum().backward()
    assert torch.isfinite(y).all() and torch.isfinite(x.grad).all()
    assert x.grad[0, 0, 2] == 0
    g, = torch.autograd.grad(lighting.srgb_encode(x).sum(), x)
    assert torch.equal(g[0, 0, :2], torch.tensor([12.92, 12.92])) and g[0, 0, 2] == 0
    z = torch.tensor([0., 12.92 * lighting.SRGB_KNEE, -0.5], requires_grad=True)
    gz, = torch.autograd.grad(lighting.srgb_decode(z).sum(), z)
    assert torch.isfinite(gz).all()


def test_decode_undoes_encode():
    """srgb_decode(srgb_encode(x)) == x to float32 rounding on [0, 1].  Above the knee the encode rounds three times (power,
    product, difference) and the decode's sum and quotient twice more: five relative errors of 2^-24 in the base of a power of
    2.4, which multiplies them, and the power's own: 5 * 2.4 + 1 = 13, allowed as 16; below the knee two roundings."""
    from dirt_amd import lighting
    x = torch.cat([torch.linspace(0., 1., 4097), torch.linspace(0., 2. * lighting.SRGB_KNEE, 1025), torch.tensor([lighting.SRGB_KNEE])])
    back = lighting.srgb_decode(lighting.srgb_encode(x))
    assert ((back - x).abs() <= 16 * 2. ** -24 * x.clamp_min(2. ** -20)).all(), float(((back - x).abs() / x.clamp_min(2. ** -20)).max())
    x64 = x.double()
    assert (lighting.srgb_decode(lighting.srgb_encode(x64)) - x64).abs().max() <= 1e-8      # (the standard's rounded constants leave its two segments 2e-9 apart at the knee)
    assert lighting.srgb_encode(torch.tensor([-1., 0., 1.])).tolist() == [0., 0., pytest.approx(1., abs=1e-7)]


def test_the_cases_keep_their_classes():
    """No case leaves more than 3 % of its elements out as kinks, and each keeps at least 8 elements floored, on the linear sRGB
    segment, above 1 before the clamp, and inside (the one-pixel shapes aside, which are there for the walk)"""
    cases = [(name, R.case(name)) for name in R.NAMES if not name.startswith('pixel')] \
        + [(name, R.Case(1000 + k, **dict(dict(curve=('aces', 'reinhard')[len(name) % 2]), **kw))) for k, (name, kw) in enumerate(SHAPES)]
    for name, c in cases:
        assert c.share <= 0.03, (name, c.share)
        classes = c.classes()
        assert min(classes.values()) >= 8, (name, classes)


def test_the_mixture_over_seeds():
    """17 x 19 x 3 over S = 1..4, the three curves and 10 seeds, in float64: at most 3 % left out, at least 8 in every class"""
    for seed in range(10):
        for S in (1, 2, 3, 4):
            for curve in R.CURVES:
                c = R.Case(5000 + seed, S=S, curve=curve)
                assert c.share <= 0.03 and min(c.classes().values()) >= 8, (seed, S, curve, c.share, c.classes())
