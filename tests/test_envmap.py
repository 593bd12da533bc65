"""The environment prefilter (dirt_amd.texture.prefilter_cube, convolve_cube, cube_pyramid, sample_cube_pyramid and their
pure-torch form cube_texel_directions / convolve_cube_dense; include/dirt_hip.h dirt_envmap_filter_forward / _backward) against
the numpy float64 restatement of DESIGN.md §7 (tests/envmap_reference.py).

Tolerance of the GPU comparisons: per element, relative to the L1 mass of the element's terms (sum of |weight| |value|), as
tests/test_texture_cube.py.  The sums here run to 6 n^2 terms, so the factor is this kernel's own: the worst error / mass over
the convolution cases of this file (`CASES` and `CHANNEL_CASES`, forward and backward) against the float64 reference, measured on
an MI355X, was MEASURED_WORST = 5.333e-7 (n = 32, roughness 0.3, forward); FACTOR = 2.13e-6 is four times that (the margin
covers a change of summation order by the compiler) and must stay within 1e-4, the project's specification tolerance.  (The other
comparisons of this file held to FACTOR reached at most 8.1e-7 in the same run: level 1 of the prefiltered 16^2 pyramid.)  The
look-up's own factor is tests/test_texture_cube.py's TOL."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import cube_reference as cr
from tests import envmap_reference as er
from tests.test_texture_cube import TOL as LOOKUP_TOL, random_dirs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED_WORST = 5.333e-7   # n = 32, roughness 0.3, forward
FACTOR = 4 * MEASURED_WORST  # 2.13e-6
SENTINEL = -7777.25
FWD, BWD = 'dirt_envmap_filter_forward', 'dirt_envmap_filter_backward'
PINNED = ('blend_', 'skin_', 'kinematics_', 'geometry_', 'shade_sh_', 'shade_pbr_', 'tangent_', 'normal_map_', 'texture_cube', 'raster_kernel', 'grad_kernel<')

# (n, roughness, kind): tiles smaller than a workgroup; exactly one tile per face; partial tiles; then n = 32 (2 x 2 tiles per face)
# with a cull that matters, at alpha = 1 / 4 where the cut-off switches off, over the hemisphere, and at the narrowest lobe
CASES = [(1, 0.5, 'ggx'), (2, 0.5, 'ggx'), (5, 0.5, 'ggx'), (16, 0.5, 'ggx'), (20, 0.5, 'ggx'), (40, 0.4, 'ggx'),
         (32, 0.3, 'ggx'), (32, 0.5, 'ggx'), (32, 1.0, 'ggx'), (32, None, 'lambert'), (32, 1 / 32, 'ggx')]
CHANNEL_CASES = [1, 3, 4, 5, 8, 9]   # every template, and the generic form with one, two and three passes (the last of them partial)


def test_the_tolerance_factor_is_within_the_specification():
    assert 0 < FACTOR <= 1e-4


def _worst(got, want, mass, what, tol):
    """Per element |got - want| <= tol * mass; -> the worst error / mass (printed: run with -s to read it)."""
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    want, mass = np.asarray(want, np.float64), np.asarray(mass, np.float64)
    assert got.shape == want.shape == mass.shape, (what, got.shape, want.shape, mass.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    ratio = float(np.max(err / (mass + 1e-30)))
    print('ENVMAP_RATIO %s: worst error / mass %.3e' % (what, ratio))
    bad = err > tol * mass + 1e-30
    if bad.any():
        worst = int(np.argmax(err - tol * mass))
        raise AssertionError('%s: %d of %d elements outside %g * mass; worst err %g at mass %g (value %g)' % (
            what, int(bad.sum()), err.size, tol, err.flat[worst], mass.flat[worst], want.flat[worst]))
    return ratio


# ---- the restatement and the torch form, on the CPU ---------------------------------------------------------------------

@pytest.mark.parametrize('size', [1, 2, 5, 16])
def test_texel_directions_map_back_to_their_texels(size):
    from dirt_amd import texture
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 4 * size * 2.0 ** -23)):
        d, w = texture.cube_texel_directions(size, dtype=dtype)
        assert tuple(d.shape) == (6, size, size, 3) and tuple(w.shape) == (6, size, size) and d.dtype == w.dtype == dtype
        face, idx, valid = texture.directions_to_cube_indices(d, size)
        f, r, c = np.meshgrid(np.arange(6), np.arange(size), np.arange(size), indexing='ij')
        assert valid.all() and np.array_equal(face.numpy(), f)
        assert np.abs(idx.numpy() - np.stack([r, c], -1)).max() <= tol
        dn, wn = er.texel_directions(size)
        assert np.abs(d.numpy() - dn).max() <= 4 * np.finfo(d.numpy().dtype).eps and np.abs(w.numpy() / wn - 1).max() <= 16 * np.finfo(d.numpy().dtype).eps
        assert np.abs(np.linalg.norm(dn, axis=-1) - 1).max() < 1e-15


@pytest.mark.parametrize('n,roughness,kind', [(5, 0.5, 'ggx'), (8, 0.2, 'ggx'), (8, 1.0, 'ggx'), (4, 1 / 32, 'ggx'), (8, None, 'lambert'), (3, 0, 'ggx')])
def test_the_dense_form_agrees_with_the_restatement(n, roughness, kind):
    """In float64 to rounding (the dense form takes 1 - t^2 from |d_o - d_s|^2, the restatement from t), with its autograd gradient
    the transpose; in float32 within the bound of a float32 sum of 6 n^2 terms, (6 n^2 + 16) 2^-24 of their mass (the 16: the weights'
    own roundings)."""
    from dirt_amd import texture
    rng = np.random.default_rng(10 + n)
    cube, g = rng.uniform(-1, 1, (6, n, n, 3)), rng.standard_normal((6, n, n, 3))
    want, mass = er.convolve(cube, roughness, kind)
    gwant, gmass = er.convolve_grad(g, roughness, kind)
    for dtype, tol in ((torch.float64, 1e-9), (torch.float32, (6 * n * n + 16) * 2.0 ** -24)):
        c_t = torch.from_numpy(cube).to(dtype).requires_grad_(True)
        out = texture.convolve_cube_dense(c_t, roughness, kind)
        assert out.dtype == dtype and out.shape == c_t.shape
        c32 = c_t.detach().numpy().astype(np.float64)
        _worst(out, *er.convolve(c32, roughness, kind), 'dense forward', tol)
        out.backward(torch.from_numpy(g).to(dtype))
        _worst(c_t.grad, gwant, gmass, 'dense backward', tol)
    assert mass.min() >= 0 and want.shape == cube.shape


def test_a_constant_cube_stays_constant():
    from dirt_amd import texture
    cube = torch.full((6, 6, 6, 2), 0.75, dtype=torch.float64)
    for roughness, kind in ((0.4, 'ggx'), (1.0, 'ggx'), (1 / 32, 'ggx'), (None, 'lambert')):
        assert (texture.convolve_cube_dense(cube, roughness, kind) - 0.75).abs().max().item() <= 1e-14
        assert np.abs(er.convolve(cube.numpy(), roughness, kind)[0] - 0.75).max() <= 1e-14


def test_the_narrowest_lobe_at_32_texels_is_the_identity():
    """roughness 1 / 32 at n = 32: in float64 only the texel itself has weight."""
    from dirt_amd import texture
    w = er.weight_matrix(32, 1 / 32, 'ggx')
    assert np.count_nonzero(w) == w.shape[0] and (np.diagonal(w) == 1).all()
    cube = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (6, 32, 32, 1)))
    assert torch.equal(texture.convolve_cube_dense(cube, 1 / 32), cube)
    assert er.live_tile_pairs(32, 1 / 32, 'ggx') == (24, 576)


def test_the_cull_cases_of_the_gpu_suite_have_something_to_cull():
    """n = 32, roughness 0.3: the reference's own live-pair count stays under half of the tile pairs (else the case tests no cull);
    the hemisphere leaves the pairs of opposite quadrants of opposite faces dead."""
    live, pairs = er.live_tile_pairs(32, 0.3, 'ggx')
    print('live tile pairs at n = 32, roughness 0.3: %d of %d' % (live, pairs))
    assert pairs == 576 and 24 < live < pairs // 2
    for roughness, kind in ((1.0, 'ggx'), (None, 'lambert')):
        live, pairs = er.live_tile_pairs(32, roughness, kind)
        print('live tile pairs at n = 32, %s %s: %d of %d' % (kind, roughness, live, pairs))
        assert pairs == 576 and 288 < live < pairs


def _cpu_pyramid(n=4, ct=3, levels=3):
    from dirt_amd import texture
    floats = sum((n >> k) ** 2 * ct for k in range(levels))
    return texture.CubePyramid(torch.zeros(6, floats), n, ct, levels)


def test_python_refusals_before_any_device_work():
    """Every refusal of the wrappers, on CPU tensors: the argument checks come first, the refusal of the CPU itself last."""
    from dirt_amd import texture
    cube = torch.zeros(6, 4, 4, 3)
    d, lod = torch.ones(5, 3), torch.zeros(5)

    def refused(text, f, *a, error=ValueError, **kw):
        with pytest.raises(error, match=text):
            f(*a, **kw)

    for f in (texture.convolve_cube, texture.convolve_cube_dense):
        name = f.__name__
        refused(name + r' expects cube to be 4D \[6, size, size, channels\], got shape \(5, 4, 4, 3\)', f, torch.zeros(5, 4, 4, 3), 0.5)
        refused(r'got shape \(6, 4, 3, 3\)', f, torch.zeros(6, 4, 3, 3), 0.5)
        refused(r'got shape \(6, 4, 4\)', f, torch.zeros(6, 4, 4), 0.5)
        refused(r'got shape \(6, 0, 0, 3\)', f, torch.zeros(6, 0, 0, 3), 0.5)
        refused(r'got shape \(\)', f, None, 0.5)
        refused(name + ': cube must be a floating-point tensor, got torch.int32', f, cube.to(torch.int32), 0.5)
        refused(name + ": kind must be 'ggx' or 'lambert', got 'phong'", f, cube, 0.5, 'phong')
        refused(name + ": roughness applies to kind='ggx' only", f, cube, 0.5, 'lambert')
        refused(name + ": kind='ggx' needs a roughness", f, cube)
        for bad in (0.01, 1.5, -0.25, float('nan'), True, '0.5', torch.tensor(0.5)):
            refused(name + r': roughness must be a float that is 0 or in \[1/32, 1\]', f, cube, bad)
    refused('convolve_cube runs on an MI355X only; there is no CPU fallback', texture.convolve_cube, cube, 0.5, error=RuntimeError)
    refused('convolve_cube runs on an MI355X only', texture.convolve_cube, cube, kind='lambert', error=RuntimeError)

    for f in (texture.cube_pyramid, texture.prefilter_cube):
        name = f.__name__
        refused(name + r' expects cube to be 4D', f, torch.zeros(6, 4, 4))
        refused(name + ': cube must be a floating-point tensor', f, cube.to(torch.int64))
        refused('max_level must be a non-negative int or None, got -1', f, cube, max_level=-1)
        refused(name + ' runs on an MI355X only; there is no CPU fallback', f, cube, error=RuntimeError)
    refused(r'prefilter_cube: roughness must be a tuple of 3 floats, one per level', texture.prefilter_cube, cube, (0.0, 0.5))
    refused(r'prefilter_cube: roughness must be a tuple of 2 floats', texture.prefilter_cube, cube, (0.0, 0.5, 1.0), max_level=1)
    refused(r'prefilter_cube: roughness must be a tuple of 3 floats', texture.prefilter_cube, cube, 0.5)
    refused(r'prefilter_cube: roughness must be a tuple of 3 floats', texture.prefilter_cube, cube, torch.zeros(3))
    refused(r'prefilter_cube: roughness must be a float that is 0 or in \[1/32, 1\], got 0.02', texture.prefilter_cube, cube, (0.0, 0.02, 1.0))

    pyr = _cpu_pyramid()
    f = texture.sample_cube_pyramid
    refused('sample_cube_pyramid expects a CubePyramid', f, pyr.packed, d, lod)
    refused(r'sample_cube_pyramid expects directions of shape \[..., 3\], got \(5, 2\)', f, pyr, torch.ones(5, 2), lod)
    refused('directions must be a floating-point tensor', f, pyr, torch.ones(5, 3, dtype=torch.int32), lod)
    refused(r'lod must be a tensor shaped like directions\[..., 0\] \(5,\), got \(4,\)', f, pyr, d, torch.zeros(4))
    refused(r'lod must be a tensor shaped like directions\[..., 0\]', f, pyr, d, None)
    refused('sample_cube_pyramid runs on an MI355X only; there is no CPU fallback', f, pyr, d, lod, error=RuntimeError)
    refused('cube_texel_directions: size must be a positive int', texture.cube_texel_directions, 0)
    refused('CubePyramid.level: level 3 of 3', pyr.level, 3)
    assert [tuple(pyr.level(k).shape) for k in range(3)] == [(6, 4, 4, 3), (6, 2, 2, 3), (6, 1, 1, 3)]
    assert pyr.level(2).data_ptr() == pyr.packed.data_ptr() + 4 * (16 + 4) * 3 and pyr.roughness is None


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_the_library_declares_builds_and_exports_the_entry_points(lib):
    from dirt_amd import build, _lib
    header = open(os.path.join(ROOT, 'include', 'dirt_hip.h')).read()
    for name in (FWD, BWD):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and re.search(r'\bint %s\(' % name, header)
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define DIRT_ENVMAP_(\w+)\s+(\d+)u', header)}
    assert consts == {'GGX': 0, 'LAMBERT': 1} and (_lib.ENVMAP_GGX, _lib.ENVMAP_LAMBERT) == (0, 1)
    assert 'dirt_envmap.hip' in build.SOURCES and 'dirt_envmap.hip' not in build.PER_SOURCE_FLAGS
    assert lib.dirt_abi_version() == 4


def test_the_source_adds_nothing_to_memory():
    text = open(os.path.join(ROOT, 'dirt_amd', 'csrc', 'dirt_envmap.hip')).read()
    assert 'atomic' not in text.lower()


def test_the_kernels_and_their_resources():
    """One template: channel counts 1, 3, 4 and any, both kinds, forward and transposed; none uses scratch memory; no name carries
    a substring by which another stage's tests count their kernels."""
    from dirt_amd import build
    res = {k: v for k, v in build.kernel_resources().items() if 'envmap_' in k}
    want = {'void dirt::envmap_filter_kernel<%d, %du, %s>' % (ct, kind, tr) for ct in (0, 1, 3, 4) for kind in (0, 1) for tr in ('false', 'true')}
    assert set(res) == want, sorted(res)
    assert all(v['scratch'] == 0 for v in res.values()), res
    assert all(v['lds'] <= 8192 for v in res.values()), res
    assert not [k for k in res for p in PINNED if p in k]


def test_c_abi_refusals_before_any_device_work(lib):
    """Every refusal of the two entry points, with pointers that are never dereferenced: the code, the message, and the rasteriser's
    error channel left as it was."""
    from dirt_amd import _lib
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(4096)
    assert lib.dirt_workspace_bytes(-1, 3, 1, 16, 16, 3) == 0
    raster_text = lib.dirt_last_error()
    assert raster_text

    def fwd(src=one, dst=two, norm=one, size=8, ch=3, stride=None, alpha=0.25, kind=0):
        return lib.dirt_envmap_filter_forward(src, dst, norm, size, ch, size * size * ch if stride is None else stride, alpha, kind, None)

    def bwd(gdst=one, norm=one, gsrc=two, size=8, ch=3, stride=None, alpha=0.25, kind=0):
        return lib.dirt_envmap_filter_backward(gdst, norm, gsrc, size, ch, size * size * ch if stride is None else stride, alpha, kind, None)

    for name, f, ptrs, same in ((FWD, fwd, ('src', 'dst', 'norm'), dict(src=one, dst=one)), (BWD, bwd, ('gdst', 'norm', 'gsrc'), dict(gdst=one, gsrc=one))):
        cases = [(dict(size=0), 'bad sizes (size=0 channels=3)'), (dict(size=-4), 'bad sizes'), (dict(ch=0), 'bad sizes (size=8 channels=0)'),
                 (dict(size=16385), 'size 16385, at most 16384'), (dict(stride=8 * 8 * 3 - 1), 'face_stride 191 is less than a level (8 x 8 x 3)'),
                 (dict(stride=-1), 'face_stride -1'), (dict(kind=2), 'kind 2 is neither DIRT_ENVMAP_GGX nor DIRT_ENVMAP_LAMBERT'),
                 (dict(alpha=0.0), 'alpha 0 is outside (0, 1]'), (dict(alpha=-0.5), 'alpha -0.5 is outside (0, 1]'),
                 (dict(alpha=1.5), 'alpha 1.5 is outside (0, 1]'), (dict(alpha=float('nan')), 'is outside (0, 1]'), (same, 'every output reads the whole level')]
        cases += [({p: None}, 'is NULL') for p in ptrs]
        for kw, text in cases:
            assert f(**kw) == _lib.E_INVALID_ARGUMENT, kw
            message = lib.dirt_texture_last_error().decode()
            assert message.startswith(name + ': ') and text in message and len(message) < 256, (kw, message)
        assert f(alpha=7.0, kind=1, **{ptrs[0]: None}) == _lib.E_INVALID_ARGUMENT
        assert 'NULL' in lib.dirt_texture_last_error().decode()     # Lambert ignores alpha: the refusal is the pointer's
    assert lib.dirt_last_error() == raster_text


# ---- on the GPU -----------------------------------------------------------------------------------------------------------

def _dev(gpu, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


def _convolve_both_ways(gpu, cube, g, roughness, kind, what):
    """convolve_cube and its backward against the reference; -> the worst error / mass of the two."""
    from dirt_amd import texture
    c_t = _dev(gpu, cube).requires_grad_(True)
    out = texture.convolve_cube(c_t, roughness, kind)
    assert out.shape == c_t.shape and out.dtype == torch.float32
    out.backward(_dev(gpu, g))
    a = _worst(out, *er.convolve(cube, roughness, kind), what + ' forward', FACTOR)
    b = _worst(c_t.grad, *er.convolve_grad(g, roughness, kind), what + ' backward', FACTOR)
    return max(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize('n,roughness,kind', CASES)
def test_convolve_cube_against_the_reference(gpu, n, roughness, kind):
    rng = np.random.default_rng(100 + n)
    cube = rng.uniform(-1, 1, (6, n, n, 3)).astype(np.float32)
    g = rng.standard_normal((6, n, n, 3)).astype(np.float32)
    if (n, roughness) == (32, 0.3):
        live, pairs = er.live_tile_pairs(n, roughness, kind)
        assert live < pairs // 2, (live, pairs)      # the case's condition: otherwise it tests no cull
    _convolve_both_ways(gpu, cube, g, roughness, kind, 'n=%d %s %s' % (n, kind, roughness))


@pytest.mark.gpu
@pytest.mark.parametrize('ct', CHANNEL_CASES)
def test_convolve_cube_with_every_channel_count(gpu, ct):
    rng = np.random.default_rng(200 + ct)
    cube = rng.uniform(-1, 1, (6, 20, 20, ct)).astype(np.float32)
    g = rng.standard_normal((6, 20, 20, ct)).astype(np.float32)
    _convolve_both_ways(gpu, cube, g, 0.5, 'ggx', 'C=%d' % ct)


@pytest.mark.gpu
def test_roughness_zero_is_a_copy(gpu):
    from dirt_amd import texture
    c_t = _dev(gpu, np.random.default_rng(5).uniform(-1, 1, (6, 5, 5, 3)).astype(np.float32)).requires_grad_(True)
    out = texture.convolve_cube(c_t, 0.0)
    g = torch.randn_like(out)
    out.backward(g)
    assert torch.equal(out, c_t) and out.data_ptr() != c_t.data_ptr() and torch.equal(c_t.grad, g)


@pytest.mark.gpu
def test_a_dead_tile_pair_is_skipped_not_summed(gpu):
    """The hemisphere at n = 32: every texel of the quadrant y > 0, z > 0 of face +X is at more than a right angle from every texel
    of the quadrant y < 0, z < 0 of face -X, so that tile pair is dropped whole -- a NaN there never reaches the sum (a pair of
    weight 0 that is summed makes it NaN).  The gradient of the dead quadrant is 0 in turn, whatever arrives at +X's."""
    from dirt_amd import texture
    rng = np.random.default_rng(6)
    cube = rng.uniform(-1, 1, (6, 32, 32, 3)).astype(np.float32)
    d = er.texel_directions(32)[0]
    assert (d[0, :16, :16, 1:] > 0).all() and (d[1, 16:, :16, 1:] < 0).all()
    assert not er.weight_matrix(32, None, 'lambert').reshape(6, 32, 32, 6, 32, 32)[0, :16, :16, 1, 16:, :16].any()
    cube[1, 16:, :16] = np.nan
    for roughness, kind in ((None, 'lambert'), (1.0, 'ggx')):
        out = texture.convolve_cube(_dev(gpu, cube), roughness, kind)
        assert torch.isfinite(out[0, :16, :16]).all() and torch.isnan(out[1, 16:, :16]).all()
        g = torch.zeros_like(out)
        g[0, :16, :16] = float('nan')
        c_t = _dev(gpu, np.nan_to_num(cube)).requires_grad_(True)
        texture.convolve_cube(c_t, roughness, kind).backward(g)
        assert not c_t.grad[1, 16:, :16].any()


@pytest.mark.gpu
def test_a_level_view_is_read_in_place(gpu):
    """A level of a packed pyramid -- faces a pyramid apart -- gives the bits of its contiguous copy, and its gradient lands in the
    level's floats of the packed buffer alone."""
    from dirt_amd import texture
    rng = np.random.default_rng(7)
    pyr = texture.cube_pyramid(_dev(gpu, rng.uniform(-1, 1, (6, 40, 40, 3)).astype(np.float32)))
    assert pyr.levels == 4 and pyr.roughness is None
    leaf = pyr.packed.detach().requires_grad_(True)
    view = texture.CubePyramid(leaf, pyr.size, pyr.channels, pyr.levels).level(1)
    assert tuple(view.shape) == (6, 20, 20, 3) and not view.is_contiguous()
    g = _dev(gpu, rng.standard_normal((6, 20, 20, 3)).astype(np.float32))
    out = texture.convolve_cube(view, 0.5)
    out.backward(g)
    copy = view.detach().contiguous().requires_grad_(True)
    out2 = texture.convolve_cube(copy, 0.5)
    out2.backward(g)
    assert torch.equal(out, out2)
    _worst(out, *er.convolve(copy.detach().cpu().numpy(), 0.5), 'level view forward', FACTOR)
    o = 40 * 40 * 3
    assert torch.equal(leaf.grad[:, o:o + 1200].reshape(6, 20, 20, 3), copy.grad)
    assert not leaf.grad[:, :o].any() and not leaf.grad[:, o + 1200:].any()


@pytest.mark.gpu
@pytest.mark.parametrize('n,ct,kind', [(20, 3, 0), (5, 4, 1), (33, 5, 0)])
def test_c_abi_writes_inside_its_outputs_only(gpu, lib, n, ct, kind):
    """Faces a stride apart with sentinels before, between and after them: dst and grad_src keep every float outside their six
    levels, norm (dense) its pads; grad_src, handed over full of garbage, comes back as the gradient alone."""
    from dirt_amd import rasterise_ops as ops
    rng = np.random.default_rng(300 + n)
    pad, level = 7, n * n * ct
    stride = level + 11
    cube = rng.uniform(-1, 1, (6, n, n, ct)).astype(np.float32)
    g = rng.standard_normal((6, n, n, ct)).astype(np.float32)
    roughness = 0.5
    stream = ops._stream_handle(gpu)

    def strided(x):
        buf = torch.full((pad + 6 * stride,), SENTINEL, device=gpu)
        if x is not None:
            buf[pad:].view(6, stride)[:, :level] = _dev(gpu, x).reshape(6, level)
        return buf

    def check_pads(buf, what):
        faces = buf[pad:].view(6, stride)
        assert (buf[:pad] == SENTINEL).all() and (faces[:, level:] == SENTINEL).all(), what
        return faces[:, :level].reshape(6, n, n, ct)

    src, dst, gdst, gsrc = strided(cube), strided(None), strided(g), strided(None)
    gsrc[pad:].view(6, stride)[:, :level] = float('nan')
    norm = torch.full((pad + 6 * n * n + pad,), SENTINEL, device=gpu)
    assert lib.dirt_envmap_filter_forward(src.data_ptr() + 4 * pad, dst.data_ptr() + 4 * pad, norm.data_ptr() + 4 * pad, n, ct, stride, roughness ** 2, kind, stream) == 0
    assert lib.dirt_envmap_filter_backward(gdst.data_ptr() + 4 * pad, norm.data_ptr() + 4 * pad, gsrc.data_ptr() + 4 * pad, n, ct, stride, roughness ** 2, kind, stream) == 0
    torch.cuda.synchronize()
    assert lib.dirt_texture_last_error() == b''
    name = ('ggx', 'lambert')[kind]
    r = None if kind else roughness
    _worst(check_pads(dst, 'dst'), *er.convolve(cube, r, name), 'C ABI forward', FACTOR)
    _worst(check_pads(gsrc, 'grad_src'), *er.convolve_grad(g, r, name), 'C ABI backward', FACTOR)
    assert (norm[:pad] == SENTINEL).all() and (norm[-pad:] == SENTINEL).all() and (norm[pad:-pad] > 0).all()
    assert torch.equal(check_pads(src, 'src'), _dev(gpu, cube)) and torch.equal(check_pads(gdst, 'grad_dst'), _dev(gpu, g))


@pytest.mark.gpu
@pytest.mark.parametrize('n,roughness,kind', [(20, 0.5, 'ggx'), (32, 0.3, 'ggx'), (32, None, 'lambert')])
def test_the_backward_is_the_transpose_of_the_forward(gpu, n, roughness, kind):
    """<g, F x> and <F^T g, x> on random x and g, each a sum of products whose factors carry the per-element bound: they agree
    within FACTOR times the summed masses of both."""
    from dirt_amd import texture
    rng = np.random.default_rng(400 + n)
    x = rng.uniform(-1, 1, (6, n, n, 3)).astype(np.float32)
    g = rng.standard_normal((6, n, n, 3)).astype(np.float32)
    x_t = _dev(gpu, x).requires_grad_(True)
    out = texture.convolve_cube(x_t, roughness, kind)
    out.backward(_dev(gpu, g))
    left = float((out.detach().cpu().numpy().astype(np.float64) * g).sum())
    right = float((x_t.grad.cpu().numpy().astype(np.float64) * x).sum())
    bound = FACTOR * (float((er.convolve(x, roughness, kind)[1] * np.abs(g)).sum()) + float((er.convolve_grad(g, roughness, kind)[1] * np.abs(x)).sum()))
    print('ENVMAP_TRANSPOSE n=%d %s: <g, F x> = %.9g, <F^T g, x> = %.9g, bound %.3g' % (n, kind, left, right, bound))
    assert abs(left - right) <= bound


@pytest.mark.gpu
def test_two_runs_give_the_same_bits(gpu):
    from dirt_amd import texture
    rng = np.random.default_rng(8)
    cube = _dev(gpu, rng.uniform(-1, 1, (6, 40, 40, 3)).astype(np.float32))
    g = _dev(gpu, rng.standard_normal((6, 40, 40, 3)).astype(np.float32))
    runs = []
    for _ in range(2):
        c_t = cube.clone().requires_grad_(True)
        out = texture.convolve_cube(c_t, 0.4)
        out.backward(g)
        pyr = texture.prefilter_cube(c_t)
        gp, = torch.autograd.grad(pyr.packed, c_t, torch.ones_like(pyr.packed))
        runs.append((out.detach(), c_t.grad, pyr.packed.detach(), gp))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def _both_look_ups(gpu, cube, d, lod, g):
    """-> [(out, grad_cube, grad_directions, grad_lod) of sample_cube_pyramid(cube_pyramid(cube), ...), of sample_texture_cube(cube, ...)]"""
    from dirt_amd import texture
    results = []
    for mine in (True, False):
        leaves = [_dev(gpu, x).requires_grad_(True) for x in (cube, d, lod)]
        if mine:
            pyr = texture.cube_pyramid(leaves[0])
            assert (pyr.size, pyr.channels, pyr.roughness) == (cube.shape[1], cube.shape[3], None)
            out = texture.sample_cube_pyramid(pyr, leaves[1], leaves[2])
        else:
            out = texture.sample_texture_cube(leaves[0], leaves[1], filter='trilinear', lod=leaves[2])
        results.append((out.detach(),) + tuple(torch.autograd.grad(out, leaves, _dev(gpu, g))))
    return results


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize('size,levels', [(12, 3), (5, 1)])
def test_a_box_pyramid_looked_up_is_sample_texture_cube_bit_for_bit(gpu, size, levels):
    """sample_cube_pyramid(cube_pyramid(cube), d, lod) runs the kernels sample_texture_cube(cube, d, 'trilinear', lod=lod) runs, on the
    same pyramid: the output and the gradients have the same bits.

    For grad_cube that can be asked only where the look-up's backward has one order of summation.  It adds to a texel with float
    atomics, so where several lanes reach one texel the bits of sample_texture_cube's own grad_cube change from run to run
    (tests/test_texture_cube.py compares two of its runs by mass, not by bits).  So: with 450 look-ups, many to a texel, the
    output, grad_directions and grad_lod (one lane each) bit for bit and grad_cube by the look-up's own rule; with one look-up
    per face -- every texel's terms come from one lane, in program order -- grad_cube bit for bit as well."""
    rng = np.random.default_rng(500 + size)
    cube = rng.uniform(-1, 1, (6, size, size, 3)).astype(np.float32)
    d = random_dirs(rng, (9, 50))
    lod = rng.uniform(-0.5, levels - 0.5, (9, 50)).astype(np.float32)
    g = rng.standard_normal((9, 50, 3)).astype(np.float32)
    mine, theirs = _both_look_ups(gpu, cube, d, lod, g)
    for a, b, name in zip(mine, theirs, ('out', 'grad_cube', 'grad_directions', 'grad_lod')):
        assert name == 'grad_cube' or _same_bits(a, b), name
    r = cr.grad(cube, d, g, 'trilinear', lod=lod)
    _worst(mine[1], r['grad_cube'], r['mass_cube'], 'box pyramid grad_cube', LOOKUP_TOL)
    _worst(theirs[1], mine[1].cpu().numpy(), r['mass_cube'], 'box pyramid grad_cube, the two paths', LOOKUP_TOL)
    assert mine[2].abs().sum() > 0 and (levels == 1 or mine[3].abs().sum() > 0)
    # one look-up per face, off the texel centres and between two levels
    faces = np.array([[1, .3, -.2], [-1, .1, .6], [.4, 1, -.7], [-.5, -1, .2], [.15, -.45, 1], [.7, .25, -1]], np.float32) * rng.uniform(0.5, 2, (6, 1)).astype(np.float32)
    lod1 = rng.uniform(0.1, max(levels - 1.1, 0.2), 6).astype(np.float32)
    g1 = rng.standard_normal((6, 3)).astype(np.float32)
    assert np.array_equal(cr.Look(faces).face, np.arange(6))
    mine, theirs = _both_look_ups(gpu, cube, faces, lod1, g1)
    for a, b, name in zip(mine, theirs, ('out', 'grad_cube', 'grad_directions', 'grad_lod')):
        assert _same_bits(a, b), 'one look-up per face: ' + name
    assert all((mine[1][f] != 0).any() for f in range(6))


def _end_to_end_reference(cube, d, lod, g, roughness=None):
    levels = er.prefilter(cube, roughness)
    roughness = er.default_roughness(len(levels)) if roughness is None else roughness
    r = er.lookup_grad(levels, d, lod, g)
    r['grad_cube'], r['mass_cube'] = er.prefilter_grad(r['grad_levels'], r['mass_levels'], roughness)
    return levels, r


def _check_end_to_end(out, gc, gd, gl, r, what):
    """The composition's bounds: a look-up reads pyramid values that are off by FACTOR of their mass and adds its own LOOKUP_TOL, so
    the output, the direction and the lod gradients are held to the sum of the two; the cube's gradient passes the look-up's
    backward, then the transposed filters."""
    tol = FACTOR + LOOKUP_TOL
    _worst(out, r['out'], r['mag'], what + ' out', tol)
    _worst(gc, r['grad_cube'], r['mass_cube'], what + ' grad_cube', tol)
    _worst(gd, r['grad_directions'], r['mass_directions'], what + ' grad_directions', tol)
    _worst(gl, r['grad_lod'], r['mass_lod'], what + ' grad_lod', tol)


@pytest.mark.gpu
def test_prefilter_then_look_up_end_to_end(gpu):
    """prefilter_cube -> sample_cube_pyramid at N = 16, C = 3 with lod across (and beyond) the five levels: the levels, the output and
    the gradients to the cube, the directions and lod against the reference's composition."""
    from dirt_amd import texture
    rng = np.random.default_rng(600)
    cube = rng.uniform(-1, 1, (6, 16, 16, 3)).astype(np.float32)
    d = random_dirs(rng, (20, 30))
    lod = rng.uniform(-0.5, 4.5, (20, 30)).astype(np.float32)
    g = rng.standard_normal((20, 30, 3)).astype(np.float32)
    leaves = [_dev(gpu, x).requires_grad_(True) for x in (cube, d, lod)]
    pyr = texture.prefilter_cube(leaves[0])
    assert pyr.levels == 5 and pyr.roughness == (0.0, 0.25, 0.5, 0.75, 1.0) and tuple(pyr.packed.shape) == (6, (256 + 64 + 16 + 4 + 1) * 3)
    out = texture.sample_cube_pyramid(pyr, leaves[1], leaves[2])
    gc, gd, gl = torch.autograd.grad(out, leaves, _dev(gpu, g))
    levels, r = _end_to_end_reference(cube, d, lod, g)
    box = er.box_levels(cube)
    for k, want in enumerate(levels):
        mass = er.convolve(box[k], pyr.roughness[k])[1]
        _worst(pyr.level(k), want, mass, 'level %d' % k, FACTOR)
    assert torch.equal(pyr.level(0), leaves[0].detach())
    _check_end_to_end(out, gc, gd, gl, r, 'end to end')
    # roughness chosen by the caller, a capped pyramid
    pyr2 = texture.prefilter_cube(leaves[0], (1 / 32, 0.6), max_level=1)
    want2 = er.prefilter(cube, (1 / 32, 0.6), max_level=1)
    assert pyr2.levels == 2 and pyr2.roughness == (1 / 32, 0.6)
    for k in range(2):
        _worst(pyr2.level(k), want2[k], er.convolve(box[k], pyr2.roughness[k])[1], 'chosen roughness level %d' % k, FACTOR)


@pytest.mark.gpu
def test_a_captured_prefilter_and_backward_replay_on_a_new_cube(gpu):
    """No host synchronisation in prefilter_cube or its backward: captured with torch.cuda.graph and replayed after the cube was
    rewritten in place, the replay matches the reference for the new contents."""
    from dirt_amd import texture
    rng = np.random.default_rng(700)
    shape = (6, 8, 8, 3)
    c_t = _dev(gpu, rng.uniform(-1, 1, shape).astype(np.float32))
    floats = (64 + 16 + 4 + 1) * 3
    g = rng.standard_normal((6, floats)).astype(np.float32)
    g_t = _dev(gpu, g)

    def step():
        leaf = c_t.detach().requires_grad_(True)
        pyr = texture.prefilter_cube(leaf)
        return pyr.packed.detach(), torch.autograd.grad(pyr.packed, leaf, g_t)[0]

    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        packed_g, gc_g = step()
    roughness = er.default_roughness(4)
    offs = np.cumsum([0, 64 * 3, 16 * 3, 4 * 3])
    for k in range(2):
        cube_k = rng.uniform(-1, 1, shape).astype(np.float32)
        with torch.no_grad():
            c_t.copy_(_dev(gpu, cube_k))
        graph.replay()
        torch.cuda.synchronize()
        box, want = er.box_levels(cube_k), er.prefilter(cube_k)
        g_levels = [g[:, o:o + lv[0].size].reshape(lv.shape).astype(np.float64) for o, lv in zip(offs, want)]
        for j, (o, lv) in enumerate(zip(offs, want)):
            _worst(packed_g[:, o:o + lv[0].size].reshape(lv.shape), lv, er.convolve(box[j], roughness[j])[1], 'replay %d level %d' % (k, j), FACTOR)
        _worst(gc_g, *er.prefilter_grad(g_levels, [np.abs(x) for x in g_levels], roughness), 'replay %d grad_cube' % k, FACTOR)


@pytest.mark.gpu
def test_the_example_fits_an_environment_through_the_prefiltered_pyramid(gpu):
    spec = importlib.util.spec_from_file_location('example_fit_environment_prefiltered', os.path.join(ROOT, 'examples', 'fit_environment_prefiltered.py'))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    losses, before, after = example.fit(width=48, height=36, steps=12, device=gpu)
    print('example: loss %.3e -> %.3e, |environment - truth| %.4f -> %.4f' % (losses[0], losses[-1], before, after))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
