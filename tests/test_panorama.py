"""`texture.panorama_to_cube` / `texture.cube_to_panorama` (dirt_panorama.hip) and their torch forms `..._dense`, by the method
of tests/test_background.py: tests/panorama_reference.py restates the specification of DESIGN.md §7k in float64; the float32
torch forms' worst |f32 - ref64| / mass per kind of result over its CASES is the F32 table below (`python -m
tests.panorama_reference` prints it), and the kernels get KERNEL times that, per element against the element's L1 mass (device
atan2 / sin / cos and the order of the sums).  An element of zero mass must be exact.

Under a rotation, output elements with a sample within 1e-3 index units of a kink (a lattice line, the u seam, an end of a
clamped index, a cube face boundary, rho == 0) are not compared and carry a zero incoming gradient: a kink bends d rotation.
Under the identity, which puts whole rows of samples on lattice lines, d rotation is not compared and only the elements where
the VALUE jumps are left out: rho == 0 (phi is set to 0 there, and a panorama's row 0 is not constant) and, for
`cube_to_panorama`, a cube face boundary (each face clamps to its own edges).  No case leaves out more than a quarter."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import panorama_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# python -m tests.panorama_reference
F32 = {'cube_out': 2.22e-4, 'cube_d_source': 4.85e-3, 'cube_d_rotation': 2.56e-7,
       'panorama_out': 1.11e-5, 'panorama_d_source': 2.31e-4, 'panorama_d_rotation': 1.63e-7}
KERNEL = 4     # the kernels' allowance over the float32 torch form
TEX_PATCH = int(re.search(r'constexpr int TEX_PATCH = (\d+);', open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_texture_common.h')).read()).group(1))


def bound(c, kind, factor=1):
    return factor * F32[('cube_' if c.to_cube else 'panorama_') + kind]


# ---- without a GPU

@pytest.mark.parametrize('name', R.CASES)
def test_the_float32_torch_form_against_the_restatement(name):
    """Per element, relative to the element's mass: within the F32 table, whose figures are this test's own worst ones"""
    c = R.case(name)
    got = R.torch_form(c)
    worst = R.ratios(got, c)
    print(name, {k: '%.2e' % v for k, v in worst.items()})
    for kind, x in worst.items():
        assert x <= bound(c, kind), (kind, x)
    assert R.exact_where_massless(got, c)


def test_the_float64_torch_form_is_the_restatement():
    """In float64 the two agree to rounding: the torch form and the restatement state one specification"""
    for name in ('n5-s3-r1', 'p5x2', 'id-n5-s3', 'q17x33', 'q-id'):
        c = R.case(name)
        worst = R.ratios(R.torch_form(c, torch.float64), c)
        assert max(worst.values()) <= 1e-9, (name, worst)


def test_no_case_leaves_out_more_than_a_quarter():
    """... and the cases of the shapes whose excluded shares were measured beforehand stay inside the measured ranges"""
    for name in R.CASES:
        assert R.case(name).share <= 0.25, (name, R.case(name).share)
    for stem, lo, hi in (('n4-s4', 0.05, 0.16), ('n5-s3', 0.02, 0.08), ('n8-s2', 0.01, 0.021), ('n17-s2', 0.015, 0.017), ('n16-s1', 0., 0.01)):
        for k in range(3):
            assert lo - 0.005 <= R.case('%s-r%d' % (stem, k)).share <= hi + 0.005, (stem, k, R.case('%s-r%d' % (stem, k)).share)


def test_the_cases_reach_the_paths_they_are_there_for():
    """The bounding box of a tile's taps overflows the LDS patch on faces of the minified case (a face is one tile there) and
    fits it on faces of others: both ways of the scatter are reached.  The seam and a pole fall inside faces"""
    def boxes(name):
        c = R.case(name)
        n, s = c.sizes, c.samples
        e = R.cube_sample_directions(n, s)[:, :16 * s, :16 * s].reshape(6, -1, 3) @ c.rotation.astype(np.float64).T      # the first tile of each face
        out = []
        for f in range(6):
            look = R.look_panorama(c.source.astype(np.float64), e[f])
            assert look['valid'].all()
            r0, r1, c0, c1 = look['box']
            out.append(int((r1.max() - r0.min() + 1) * (c1.max() - c0.min() + 1)))
        return out

    assert max(boxes('minify')) > TEX_PATCH
    assert min(boxes('n16-s1-r0')) <= TEX_PATCH < max(boxes('n16-s1-r0'))      # a face away from seam and poles fits; one on them does not
    assert max(boxes('n5-s3-r1')) <= TEX_PATCH                                  # a small panorama fits whole
    # the panorama's pole (0, 1, 0) and seam direction (0, 0, 1), in the cube's frame under rotation 2, fall strictly inside a face
    for axis in ((0., 1., 0.), (0., 0., 1.)):
        d = np.abs(np.asarray(axis) @ R.rotation_matrix(R.ROTATIONS[2]).astype(np.float64))
        assert np.sort(d)[1] / d.max() < 0.9
    first, last = R.case('n17-s2-r0').source[:, 0], R.case('n17-s2-r0').source[:, -1]
    assert np.abs(first - last).min() > 0      # a wrap that took the wrong column would show


def test_texel_directions_map_back_to_their_indices():
    from dirt_amd import texture
    for H, W in ((1, 1), (3, 5), (16, 32), (7, 13)):
        d, w = texture.panorama_texel_directions(H, W, dtype=torch.float64)
        assert d.shape == (H, W, 3) and w.shape == (H, W)
        assert torch.allclose(d.norm(dim=-1), torch.ones(H, W, dtype=torch.float64), atol=1e-14)
        idx, valid = texture.directions_to_panorama_indices(d, H, W)
        rows, cols = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
        assert valid.all() and torch.allclose(idx, torch.stack([rows, cols], -1), atol=1e-10)
        assert torch.allclose(w, torch.sin(np.pi * (rows + 0.5) / H), atol=1e-14)
    d2, _ = texture.panorama_texel_directions(3, 5, samples=2, dtype=torch.float64)
    np.testing.assert_allclose(d2.numpy(), R.panorama_sample_directions(3, 5, 2), atol=1e-14)
    np.testing.assert_allclose(texture._cube_sample_directions(5, 3, None, torch.float64).numpy(), R.cube_sample_directions(5, 3), atol=1e-14)
    centres, _ = texture.cube_texel_directions(5, dtype=torch.float64)
    e = torch.from_numpy(R.cube_sample_directions(5, 1))
    assert torch.allclose(e / e.norm(dim=-1, keepdim=True), centres, atol=1e-14)      # the table of cube_texel_directions


def test_the_samples_of_a_texel_are_the_texels_of_the_finer_cube():
    """panorama_to_cube(p, N, samples=2 S) is the 2 x 2 box mean of panorama_to_cube(p, 2 N, samples=S): one sample set.  This
    pins the sample positions"""
    rng = np.random.default_rng(5)
    pan = rng.standard_normal((7, 13, 3))
    rot = R.rotation_matrix(R.ROTATIONS[0])
    for N, S in ((3, 1), (4, 2), (5, 1)):
        coarse = R.panorama_to_cube(pan, N, 2 * S, rot)['out']
        fine = R.panorama_to_cube(pan, 2 * N, S, rot)['out']
        np.testing.assert_allclose(coarse, fine.reshape(6, N, 2, N, 2, 3).mean((2, 4)), rtol=0, atol=1e-12)
    cube = rng.standard_normal((6, 4, 4, 3))
    coarse, fine = R.cube_to_panorama(cube, 3, 5, 2, rot)['out'], R.cube_to_panorama(cube, 6, 10, 1, rot)['out']
    np.testing.assert_allclose(coarse, fine.reshape(3, 2, 5, 2, 3).mean((1, 3)), rtol=0, atol=1e-12)


def test_a_constant_panorama_gives_a_constant_cube_and_panorama():
    from dirt_amd import texture
    value = torch.tensor([0.25, -1.5, 3.])
    rot = torch.from_numpy(R.rotation_matrix(R.ROTATIONS[1]))
    cube = texture.panorama_to_cube_dense(value.expand(6, 11, 3), 5, samples=3, rotation=rot)
    assert cube.shape == (6, 5, 5, 3) and torch.allclose(cube, value.expand(6, 5, 5, 3), atol=1e-6)
    pan = texture.cube_to_panorama_dense(cube, 4, 9, samples=2, rotation=rot)
    assert pan.shape == (4, 9, 3) and torch.allclose(pan, value.expand(4, 9, 3), atol=1e-6)
    ref = R.cube_to_panorama(R.panorama_to_cube(np.ones((3, 4, 2)), 4, 2, rot.numpy())['out'], 5, 3, 3, rot.numpy())['out']
    np.testing.assert_allclose(ref, 1., atol=1e-14)


def test_straight_up_takes_the_middle_column():
    """rho == 0: phi is 0, u = 0.5, and no gradient reaches the direction.  With N S odd and the identity the centre sample of
    the +Y and -Y faces is that direction exactly"""
    from dirt_amd import texture
    d = torch.tensor([[0., 2., 0.], [0., -3., 0.], [0., 0., 0.], [float('nan'), 1., 0.]], requires_grad=True)
    idx, valid = texture.directions_to_panorama_indices(d, 6, 11)
    assert valid.tolist() == [True, True, False, False]
    assert idx.tolist() == [[0., 5.], [5., 5.], [0., 0.], [0., 0.]]
    pan = torch.randn(6, 11, 2, requires_grad=True)
    texture.sample_panorama(pan, idx, valid).sum().backward()
    assert not d.grad.any() and torch.isfinite(pan.grad).all()
    c = R.case('id-n5-s3')
    jump = c.ref['jump']
    assert jump.sum() == 2 and jump[2, 2, 2] and jump[3, 2, 2]
    look = R.look_panorama(c.source.astype(np.float64), np.array([[0., 1., 0.]]))
    np.testing.assert_allclose(look['value'][0], c.source[0, 6], atol=0)      # row 0, column (0.5 * 13 - 0.5) = 6


def test_none_is_the_identity_in_the_torch_forms():
    from dirt_amd import texture
    pan, cube = torch.randn(7, 13, 3), torch.randn(6, 4, 4, 3)
    assert torch.equal(texture.panorama_to_cube_dense(pan, 5, 2), texture.panorama_to_cube_dense(pan, 5, 2, torch.eye(3)))
    assert torch.equal(texture.cube_to_panorama_dense(cube, 3, 5, 2), texture.cube_to_panorama_dense(cube, 3, 5, 2, torch.eye(3)))


PAN, CUBE = torch.zeros(4, 8, 3), torch.zeros(6, 4, 4, 3)
TO_CUBE_REFUSALS = [
    (dict(panorama=torch.zeros(4, 8)), 'panorama_to_cube expects panorama to be 3D [height, width, channels], got (4, 8)'),
    (dict(panorama=torch.zeros(4, 0, 3)), 'panorama_to_cube expects panorama to be 3D [height, width, channels], got (4, 0, 3)'),
    (dict(panorama=[1, 2]), 'panorama_to_cube expects panorama to be 3D [height, width, channels], got list'),
    (dict(panorama=torch.zeros(4, 8, 3, dtype=torch.int32)), 'panorama_to_cube: panorama must be a floating-point tensor, got torch.int32'),
    (dict(size=0), 'panorama_to_cube: size must be a positive int, got 0'),
    (dict(size=4.), 'panorama_to_cube: size must be a positive int, got 4.0'),
    (dict(size=True), 'panorama_to_cube: size must be a positive int, got True'),
    (dict(samples=0), 'panorama_to_cube: samples must be an int in 1..4, got 0'),
    (dict(samples=5), 'panorama_to_cube: samples must be an int in 1..4, got 5'),
    (dict(rotation=torch.zeros(4, 4)), 'panorama_to_cube: rotation must be a floating-point tensor [3, 3] or None, got torch.float32 (4, 4)'),
    (dict(rotation=torch.zeros(3, 3, dtype=torch.int64)), 'panorama_to_cube: rotation must be a floating-point tensor [3, 3] or None, got torch.int64 (3, 3)'),
    (dict(rotation=(1., 2., 3.)), 'panorama_to_cube: rotation must be a floating-point tensor [3, 3] or None, got tuple'),
    (dict(rotation=torch.eye(3, device='meta')), 'panorama_to_cube: rotation is on meta, the panorama on cpu'),
]
TO_PANORAMA_REFUSALS = [
    (dict(cube=torch.zeros(6, 4, 5, 3)), 'cube_to_panorama expects cube to be 4D [6, size, size, channels], got (6, 4, 5, 3)'),
    (dict(cube=torch.zeros(5, 4, 4, 3)), 'cube_to_panorama expects cube to be 4D [6, size, size, channels], got (5, 4, 4, 3)'),
    (dict(cube=None), 'cube_to_panorama expects cube to be 4D [6, size, size, channels], got NoneType'),
    (dict(cube=CUBE.to(torch.bool)), 'cube_to_panorama: cube must be a floating-point tensor, got torch.bool'),
    (dict(height=0), 'cube_to_panorama: height must be a positive int, got 0'),
    (dict(width=-3), 'cube_to_panorama: width must be a positive int, got -3'),
    (dict(samples=2.), 'cube_to_panorama: samples must be an int in 1..4, got 2.0'),
    (dict(rotation=torch.zeros(3)), 'cube_to_panorama: rotation must be a floating-point tensor [3, 3] or None, got torch.float32 (3,)'),
    (dict(rotation=torch.eye(3, device='meta')), 'cube_to_panorama: rotation is on meta, the cube on cpu'),
]


@pytest.mark.parametrize('change, text', TO_CUBE_REFUSALS, ids=[str(i) for i in range(len(TO_CUBE_REFUSALS))])
def test_python_refusals_of_panorama_to_cube_in_full(change, text):
    """Every refusal with its full text, before any device work, from the fused function and from its dense form alike"""
    from dirt_amd import texture
    kw = dict(dict(panorama=PAN, size=4, samples=1, rotation=None), **change)
    for f, who in ((texture.panorama_to_cube, 'panorama_to_cube'), (texture.panorama_to_cube_dense, 'panorama_to_cube_dense')):
        with pytest.raises(ValueError) as e:
            f(kw['panorama'], kw['size'], samples=kw['samples'], rotation=kw['rotation'])
        assert str(e.value) == text.replace('panorama_to_cube', who, 1)


@pytest.mark.parametrize('change, text', TO_PANORAMA_REFUSALS, ids=[str(i) for i in range(len(TO_PANORAMA_REFUSALS))])
def test_python_refusals_of_cube_to_panorama_in_full(change, text):
    from dirt_amd import texture
    kw = dict(dict(cube=CUBE, height=4, width=8, samples=1, rotation=None), **change)
    for f, who in ((texture.cube_to_panorama, 'cube_to_panorama'), (texture.cube_to_panorama_dense, 'cube_to_panorama_dense')):
        with pytest.raises(ValueError) as e:
            f(kw['cube'], kw['height'], kw['width'], samples=kw['samples'], rotation=kw['rotation'])
        assert str(e.value) == text.replace('cube_to_panorama', who, 1)


def test_the_helpers_refuse_in_full():
    from dirt_amd import texture
    for call, text in ((lambda: texture.panorama_texel_directions(0, 4), 'panorama_texel_directions: height must be a positive int, got 0'),
                       (lambda: texture.panorama_texel_directions(4, 4, samples=5), 'panorama_texel_directions: samples must be an int in 1..4, got 5'),
                       (lambda: texture.directions_to_panorama_indices(torch.zeros(4, 2), 4, 8),
                        'directions_to_panorama_indices expects floating-point directions of shape [..., 3], got (4, 2)'),
                       (lambda: texture.directions_to_panorama_indices(torch.zeros(4, 3), 4, 0), 'directions_to_panorama_indices: width must be a positive int, got 0')):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text


def test_what_passes_the_checks_needs_the_gpu():
    from dirt_amd import texture
    with pytest.raises(RuntimeError) as e:
        texture.panorama_to_cube(PAN.double()[:, ::2], 4, samples=4, rotation=torch.eye(3).t())
    assert str(e.value) == 'dirt_amd.texture.panorama_to_cube runs on an MI355X only; there is no CPU fallback'
    with pytest.raises(RuntimeError) as e:
        texture.cube_to_panorama(CUBE, 1, 1, samples=2)
    assert str(e.value) == 'dirt_amd.texture.cube_to_panorama runs on an MI355X only; there is no CPU fallback'


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import _lib
    return _lib.load()


FWD = dict(source=None, rotation=None, out=None, rows=4, cols=8, size=4, channels=3, samples=2, stream=None)
BWD = dict(source=None, rotation=None, grad_out=None, grad_source=None, grad_rotation=None, scratch=None, scratch_bytes=0,
           **{k: FWD[k] for k in list(FWD)[3:]})
ONE = ctypes.c_void_p(16)      # a pointer that is not NULL and is never dereferenced: every call it is given to is refused first
C_REFUSALS = [
    (dict(rows=0), '%s: bad sizes (rows=0 cols=8 size=4 channels=3), each at least 1'),
    (dict(cols=-1), '%s: bad sizes (rows=4 cols=-1 size=4 channels=3), each at least 1'),
    (dict(size=0), '%s: bad sizes (rows=4 cols=8 size=0 channels=3), each at least 1'),
    (dict(channels=0), '%s: bad sizes (rows=4 cols=8 size=4 channels=0), each at least 1'),
    (dict(samples=0), '%s: samples=0, 1..4'),
    (dict(samples=5), '%s: samples=5, 1..4'),
    (dict(size=32769), '%s: cube size 32769, at most 32768'),
    (dict(rows=(1 << 20) + 1), '%s: panorama of 1048577 x 8, at most 1048576 each way'),
    (dict(channels=65537), '%s: 65537 channels, at most 65536'),
]
NAMES = ('dirt_panorama_to_cube', 'dirt_cube_to_panorama')


def texture_error():
    from dirt_amd import _lib
    return _lib.load().dirt_texture_last_error().decode()


def test_c_refusals_come_before_any_device_work(lib):
    """Every refusal returns DIRT_E_INVALID_ARGUMENT with its sentence in dirt_texture_last_error() -- on a machine without a GPU,
    with NULL pointers: nothing was dereferenced and nothing was launched.  The backward shares the checks and adds its own."""
    from dirt_amd import _lib
    for change, text in C_REFUSALS:
        for stem in NAMES:
            for name, base in ((stem + '_forward', FWD), (stem + '_backward', BWD)):
                assert getattr(lib, name)(*dict(base, **change).values()) == _lib.E_INVALID_ARGUMENT, (name, change)
                assert texture_error() == text % name, (texture_error(), text % name)
    big = dict(rows=1 << 20, cols=1 << 20, samples=4)      # 2^22 x 2^22 samples: 2^36 tiles
    for name, base in (('dirt_cube_to_panorama_forward', FWD), ('dirt_cube_to_panorama_backward', BWD)):
        assert getattr(lib, name)(*dict(base, **big).values()) == _lib.E_INVALID_ARGUMENT
        assert texture_error() == '%s: grid too large (rows=1048576 cols=1048576 samples=4): more than 2^31 - 1 tiles' % name
    assert lib.dirt_panorama_scratch_bytes(1 << 20, 1 << 20, 4, 3, 4, 0) == 0
    assert lib.dirt_panorama_to_cube_forward(*FWD.values()) == _lib.E_INVALID_ARGUMENT
    assert texture_error() == 'dirt_panorama_to_cube_forward: panorama / rotation / cube is NULL'
    assert lib.dirt_cube_to_panorama_forward(*FWD.values()) == _lib.E_INVALID_ARGUMENT
    assert texture_error() == 'dirt_cube_to_panorama_forward: cube / rotation / panorama is NULL'
    for stem in NAMES:      # no gradient wanted: success, nothing is launched
        assert getattr(lib, stem + '_backward')(*BWD.values()) == 0 and texture_error() == ''
    given = dict(source=ONE, rotation=ONE, grad_out=ONE)
    who = 'dirt_panorama_to_cube_backward'
    need = lib.dirt_panorama_scratch_bytes(4, 8, 4, 3, 2, 1)
    assert need == 4 * 6 * 1 * 9      # a row of 9 sums per tile of each face
    assert lib.dirt_panorama_scratch_bytes(4, 8, 17, 3, 2, 1) == 4 * 6 * 4 * 9
    for change, text in [(dict(grad_source=ONE), '%s: panorama / rotation / grad_cube is NULL' % who),
                         (dict(given, grad_rotation=ONE), '%s: scratch is NULL or smaller than dirt_panorama_scratch_bytes (0 < %d)' % (who, need)),
                         (dict(given, grad_rotation=ONE, scratch=ONE, scratch_bytes=need - 4),
                          '%s: scratch is NULL or smaller than dirt_panorama_scratch_bytes (%d < %d)' % (who, need - 4, need)),
                         (dict(given, grad_rotation=ONE, scratch=ctypes.c_void_p(18), scratch_bytes=need), '%s: scratch is not 4-byte aligned' % who)]:
        assert lib.dirt_panorama_to_cube_backward(*dict(BWD, **change).values()) == _lib.E_INVALID_ARGUMENT, change
        assert texture_error() == text, (texture_error(), text)
    who = 'dirt_cube_to_panorama_backward'
    need = lib.dirt_panorama_scratch_bytes(4, 8, 4, 3, 2, 0)
    assert need == 4 * (1 * 9 + 8 * 16 * (3 + 3))      # a row per tile, then per sample its direction and what arrives at it
    assert lib.dirt_panorama_scratch_bytes(1, 300, 4, 5, 1, 0) == 4 * (2 * 9 + 300 * 8)
    for change, text in [(dict(grad_rotation=ONE), '%s: cube / rotation / grad_panorama is NULL' % who),
                         (dict(given, grad_source=ONE), '%s: scratch is NULL or smaller than dirt_panorama_scratch_bytes (0 < %d)' % (who, need)),
                         (dict(given, grad_rotation=ONE, scratch=ONE, scratch_bytes=need - 4),
                          '%s: scratch is NULL or smaller than dirt_panorama_scratch_bytes (%d < %d)' % (who, need - 4, need)),
                         (dict(given, grad_source=ONE, scratch=ctypes.c_void_p(18), scratch_bytes=need), '%s: scratch is not 4-byte aligned' % who)]:
        assert lib.dirt_cube_to_panorama_backward(*dict(BWD, **change).values()) == _lib.E_INVALID_ARGUMENT, change
        assert texture_error() == text, (texture_error(), text)
    for bad in ((0, 8, 4, 3, 2, 1), (4, 8, 0, 3, 2, 0), (4, 8, 4, 0, 2, 1), (4, 8, 4, 3, 5, 0), (4, 8, 32769, 3, 1, 1), ((1 << 20) + 1, 8, 4, 3, 1, 0)):
        assert lib.dirt_panorama_scratch_bytes(*bad) == 0, bad


def test_names_header_and_build():
    """The functions under both package names, the header's declarations, the unit in the build without flags of its own"""
    import dirt
    import dirt.texture
    import dirt_amd
    from dirt_amd import _lib, build, texture
    for name in ('panorama_to_cube', 'cube_to_panorama', 'panorama_to_cube_dense', 'cube_to_panorama_dense', 'panorama_texel_directions',
                 'directions_to_panorama_indices', 'sample_panorama'):
        assert getattr(dirt.texture, name) is getattr(dirt_amd.texture, name) is getattr(texture, name)
    assert 'dirt_panorama.hip' in build.SOURCES and 'dirt_panorama.hip' not in build.PER_SOURCE_FLAGS
    header = open(os.path.join(ROOT, 'include', 'dirt_hip.h')).read()
    for name in ('dirt_panorama_scratch_bytes',) + tuple(stem + end for stem in NAMES for end in ('_forward', '_backward')):
        assert re.search(r'\b%s\(' % name, header) and name in _lib.SYMBOLS
    assert '#define DIRT_ABI_VERSION 4' in header and _lib.ABI_VERSION == 4
    assert re.search(r'#define DIRT_PANORAMA_MAX_SAMPLES 4\b', header) and _lib.PANORAMA_MAX_SAMPLES == 4


# ---- on the GPU: the kernels against the restatement

def _dev(gpu, x):
    return torch.as_tensor(np.ascontiguousarray(x), device=gpu)


def run_kernel(c, gpu, want=(True, True), source=None, rotation=None, go=None):
    """`texture.panorama_to_cube` / `cube_to_panorama` on the case -> the keys of `R.torch_form` (a gradient that is not
    wanted is absent).  `source`, `rotation`: tensors to pass in place of the case's (views of the same values)"""
    from dirt_amd import texture
    src = _dev(gpu, c.source).requires_grad_(want[0]) if source is None else source
    rot = _dev(gpu, c.rotation).requires_grad_(want[1]) if rotation is None else rotation
    if c.to_cube:
        out = texture.panorama_to_cube(src, c.sizes, samples=c.samples, rotation=rot)
    else:
        out = texture.cube_to_panorama(src, c.sizes[0], c.sizes[1], samples=c.samples, rotation=rot)
    res = {'out': out.detach().cpu().numpy()}
    leaves = [(k, x) for k, x, on in (('d_source', src, want[0]), ('d_rotation', rot, want[1])) if on]
    if leaves:
        grads = torch.autograd.grad(out, [x for _, x in leaves], _dev(gpu, c.go) if go is None else go)
        res.update({k: g.cpu().numpy() for (k, _), g in zip(leaves, grads)})
    return res


def _check(got, c):
    worst = R.ratios(got, c)
    print({k: '%.2e' % v for k, v in worst.items()})
    for kind, x in worst.items():
        assert x == x and x <= bound(c, kind, KERNEL), (kind, x, bound(c, kind, KERNEL))
    assert R.exact_where_massless(got, c)
    assert all(np.isfinite(v).all() for v in got.values())
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('name', R.CASES)
def test_kernels_against_the_restatement(gpu, name):
    c = R.case(name)
    got = run_kernel(c, gpu)
    assert got['out'].shape == c.ref['out'].shape and got['d_source'].shape == c.source.shape and got['d_rotation'].shape == (3, 3)
    _check(got, c)


@pytest.mark.gpu
def test_no_rotation_is_the_identity_to_the_bit(gpu):
    from dirt_amd import texture
    for name in ('id-n5-s3', 'id-n17-s2', 'q-id'):
        c = R.case(name)
        src, eye, go = _dev(gpu, c.source).requires_grad_(True), torch.eye(3, device=gpu), _dev(gpu, c.go)
        if c.to_cube:
            a, b = (texture.panorama_to_cube(src, c.sizes, samples=c.samples, rotation=r) for r in (None, eye))
        else:
            a, b = (texture.cube_to_panorama(src, *c.sizes, samples=c.samples, rotation=r) for r in (None, eye))
        assert torch.equal(a, b)
        ga, gb = (torch.autograd.grad(x, src, go)[0].cpu().numpy() for x in (a, b))
        mass = c.ref['mass_d_source']
        assert R.worst_ratio(ga, gb.astype(np.float64), mass) <= bound(c, 'd_source', KERNEL)      # (float atomics: not the same bits)


@pytest.mark.gpu
def test_operands_that_are_not_contiguous(gpu):
    """A panorama that is every second column of a wider one, a cube that is a slice of more channels, a transposed rotation:
    the values of the case, by other strides"""
    for name in ('n5-s3-r1', 'q17x33'):
        c = R.case(name)
        wide = torch.zeros(c.source.shape[:-2] + (2 * c.source.shape[-2], c.source.shape[-1] + 2), device=gpu)
        view = wide[..., ::2, 1:-1]
        view.copy_(_dev(gpu, c.source))
        rot_t = _dev(gpu, c.rotation.T.copy())
        assert not view.is_contiguous() and not rot_t.t().is_contiguous()
        src, rot = view.detach().requires_grad_(True), rot_t.t().detach().requires_grad_(True)
        got = run_kernel(c, gpu, source=src, rotation=rot)
        assert got['d_source'].shape == c.source.shape
        _check(got, c)


WANTS = [(True, False), (False, True), (True, True), (False, False)]


@pytest.mark.gpu
@pytest.mark.parametrize('want', WANTS, ids=[''.join('sr'[i] if w else '-' for i, w in enumerate(want)) for want in WANTS])
def test_every_pattern_of_wanted_gradients(gpu, want):
    for name in ('n17-s2-r1', 'minify', 'q17x33'):
        c = R.case(name)
        got = run_kernel(c, gpu, want)
        assert [k for k in R.KINDS[1:] if k in got] == [k for k, w in zip(R.KINDS[1:], want) if w]
        _check(got, c)


@pytest.mark.gpu
def test_two_runs_agree(gpu):
    """d rotation and the values to the bit; the sampled operand's gradient, summed with float atomics, within the allowance"""
    for name in ('n17-s2-r2', 'n16-s1-r0', 'minify', 'q17x33', 'q1x300'):
        c = R.case(name)
        a, b = run_kernel(c, gpu), run_kernel(c, gpu)
        assert np.array_equal(a['out'], b['out']) and np.array_equal(a['d_rotation'], b['d_rotation']), name
        assert R.worst_ratio(a['d_source'], b['d_source'].astype(np.float64), c.ref['mass_d_source']) <= bound(c, 'd_source', KERNEL)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['n17-s2-r0', 'c5', 'minify', 'q17x33', 'q-c5'])
def test_c_abi_with_guard_values_around_every_output(gpu, lib, name):
    """The entry points called as C would, every output and the scratch inside a larger buffer of a guard value: nothing outside
    is written; then with each gradient pointer NULL in turn, which leaves the other's result as it was (d rotation: to the bit)"""
    from dirt_amd import texture
    c = R.case(name)
    src, rot, go = (_dev(gpu, x) for x in (c.source, c.rotation, c.go))
    pad, guard = 37, -77.25
    stem = NAMES[0] if c.to_cube else NAMES[1]
    rows, cols = c.source.shape[:2] if c.to_cube else c.sizes
    size, ct = (c.sizes if c.to_cube else c.source.shape[1]), c.source.shape[-1]
    tail = (rows, cols, size, ct, c.samples, None)

    def guarded(count):
        return torch.full((count + 2 * pad,), guard, dtype=torch.float32, device=gpu)

    def inner(t, count):
        assert (t[:pad] == guard).all() and (t[pad + count:] == guard).all()
        return t[pad:pad + count]

    at = lambda t: t.data_ptr() + 4 * pad   # noqa: E731
    n_out = int(np.prod(c.ref['out'].shape))
    nbytes = lib.dirt_panorama_scratch_bytes(rows, cols, size, ct, c.samples, int(c.to_cube))
    assert nbytes > 0
    results = []
    for want in ((True, True), (True, False), (False, True)):
        out, d_src, d_rot, scratch = guarded(n_out), guarded(src.numel()), guarded(9), guarded(nbytes // 4)
        texture._check(getattr(lib, stem + '_forward')(src.data_ptr(), rot.data_ptr(), at(out), *tail))
        texture._check(getattr(lib, stem + '_backward')(src.data_ptr(), rot.data_ptr(), go.data_ptr(), at(d_src) if want[0] else None,
                                                        at(d_rot) if want[1] else None, at(scratch), nbytes, *tail))
        torch.cuda.synchronize()
        inner(scratch, nbytes // 4)
        got = {'out': inner(out, n_out).cpu().numpy().reshape(c.ref['out'].shape)}
        for kind, t, on, shape in (('d_source', d_src, want[0], c.source.shape), ('d_rotation', d_rot, want[1], (3, 3))):
            values = inner(t, int(np.prod(shape))).cpu().numpy().reshape(shape)
            if on:
                got[kind] = values
            else:
                assert (values == guard).all()
        _check(got, c)
        results.append(got)
    assert np.array_equal(results[0]['d_rotation'], results[2]['d_rotation']) and np.array_equal(results[0]['out'], results[1]['out'])


@pytest.mark.gpu
def test_a_round_trip_returns_a_smooth_environment(gpu):
    """panorama -> cube -> panorama under one rotation returns a band-limited panorama up to the two resamplings' error, which
    the same round trip in the float64 restatement has too: the two routes agree to the kernels' allowance"""
    from dirt_amd import texture
    H, W, N = 16, 32, 32
    d = R.panorama_sample_directions(H, W, 1)
    pan = np.stack([1. + d[..., 0], 0.5 + d[..., 1] * d[..., 2], d[..., 1]], -1).astype(np.float32)
    rot = R.rotation_matrix(R.ROTATIONS[0])
    cube = texture.panorama_to_cube(_dev(gpu, pan), N, samples=2, rotation=_dev(gpu, rot))
    back = texture.cube_to_panorama(cube, H, W, samples=2, rotation=_dev(gpu, rot)).cpu().numpy()
    ref_cube = R.panorama_to_cube(pan, N, 2, rot)
    ref = R.cube_to_panorama(ref_cube['out'], H, W, 2, rot)
    worst = KERNEL * (F32['cube_out'] * ref_cube['mass_out'].max() + F32['panorama_out'] * ref['mass_out'].max())
    assert np.abs(back - ref['out']).max() <= worst
    assert np.abs(ref['out'] - pan).max() <= 0.1      # ... and both are the panorama again, to what two bilinear resamplings blur


@pytest.mark.gpu
def test_end_to_end_at_the_head_of_the_environment_chain(gpu):
    """The chain of examples/fit_environment_rotation_fused.py at 32 x 32: panorama -> panorama_to_cube(rotation) ->
    prefilter_cube -> environment_background -> resolve_image -> loss, against the same chain with the dense torch form at its
    head.  Everything after the head is linear in the cube with weights that are non-negative and sum to at most 1 (a
    normalised convolution, a trilinear look-up, a box mean), so the images differ by at most what the two cubes do: (1 + KERNEL)
    F32 of the largest mass, plus float32 rounding of the stages behind.  Gradients reach the panorama and the rotation; the
    panorama's agree in direction, the rotation's to 1e-2 of its norm (a share of the order of 1e-3 of the samples sits where
    the two float32 routes may pick neighbouring texels, and a texel step changes a sample's derivative by its own size)."""
    from dirt_amd import matrices, shading, texture
    rng = np.random.default_rng(7)
    pan = rng.uniform(0., 1., (16, 32, 3)).astype(np.float32)
    w = torch.tensor([0.3, -0.5, 0.2], device=gpu)
    target = torch.from_numpy(rng.uniform(0., 1., (32, 32, 3)).astype(np.float32)).to(gpu)
    inverse = torch.linalg.inv(matrices.perspective_projection(0.1, 10., 0.1, 1.)).to(torch.float32).to(gpu)

    def chain(head):
        p = _dev(gpu, pan).requires_grad_(True)
        v = w.clone().requires_grad_(True)
        cube = head(p, 16, samples=2, rotation=matrices.rodrigues(v, three_by_three=True))
        pyramid = texture.prefilter_cube(cube)
        behind = shading.environment_background(pyramid, inverse, (64, 64), filter='trilinear', lod=1.)
        image = shading.resolve_image(behind, factor=2, clamp=None)
        loss = ((image - target) ** 2).mean()
        loss.backward()
        return image.detach(), loss.item(), p.grad, v.grad

    fused, dense = chain(texture.panorama_to_cube), chain(lambda p, n, samples, rotation: texture.panorama_to_cube_dense(p, n, samples, rotation))
    assert fused[0].shape == (32, 32, 3)
    assert (fused[0] - dense[0]).abs().max().item() <= (1 + KERNEL) * F32['cube_out'] * 1. + 1e-5
    assert abs(fused[1] - dense[1]) <= 1e-4 * dense[1]
    for g in fused[2:]:
        assert torch.isfinite(g).all() and g.abs().sum() > 0
    cosine = torch.nn.functional.cosine_similarity(fused[2].flatten(), dense[2].flatten(), dim=0).item()
    assert cosine >= 0.999, cosine
    assert (fused[3] - dense[3]).norm() <= 1e-2 * dense[3].norm(), (fused[3], dense[3])
