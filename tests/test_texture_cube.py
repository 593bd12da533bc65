"""The cube-map look-up (dirt_amd.texture.sample_texture_cube and its pure-torch form directions_to_cube_indices / sample_cube;
include/dirt_hip.h dirt_texture_cube_forward / _backward) against the numpy restatement of DESIGN.md §7 (tests/cube_reference.py),
and the restatement itself against hand-computed values and finite differences on the CPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import cube_reference as cr
from tests import mip_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5   # per element, relative to the L1 mass of the element's terms (forward: to the blend's magnitude); tests/test_texture_mip.py's
FWD, BWD = 'dirt_texture_cube_forward', 'dirt_texture_cube_backward'
SENTINEL = -7777.25


def dirs_from_indices(face, row, col, size, a=1.0):
    """The direction that lands on fractional (row, col) of `face` of a cube of `size`, its major component of magnitude a (float64)."""
    face, row, col, a = (np.asarray(x, np.float64) for x in np.broadcast_arrays(face, row, col, a))
    sc, tc = (2. * (col + 0.5) / size - 1.) * a, (2. * (row + 0.5) / size - 1.) * a
    f = face.astype(np.int64)
    x = np.choose(f, [a, -a, sc, sc, sc, -sc])
    y = np.choose(f, [-tc, -tc, a, -a, -tc, -tc])
    z = np.choose(f, [-sc, sc, tc, -tc, a, -a])
    return np.stack([x, y, z], -1)


def random_dirs(rng, shape):
    """Directions of every face and many lengths; one in 16 is invalid, a tie or a corner."""
    d = rng.standard_normal(shape + (3,)) * np.exp(rng.uniform(-3, 3, shape + (1,)))
    d = d.astype(np.float32).reshape(-1, 3)
    pool = np.array([[0, 0, 0], [np.nan, 1, 0], [1, np.inf, 0], [0, 2, -np.inf], [1, 1, 0], [0, 1, 1], [-1, 0, 1], [1, 1, 1], [-1, -1, -1],
                     [1, -1, 1], [0, 0, -3], [0, -2, 0], [2, 0, 0], [-0.5, 0.5, 0.5], [0, 0, 4], [0, -1, 1]], np.float32)
    where = np.arange(3, len(d), 16)
    d[where] = pool[np.arange(len(where)) % len(pool)]
    return d.reshape(shape + (3,))


# ---- the restatement and the torch form, on the CPU ---------------------------------------------------------------------

AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


@pytest.mark.parametrize('size', [1, 4, 5])
def test_hand_values_of_faces_and_indices(size):
    from dirt_amd import texture
    face, idx, valid = cr.cube_indices(np.array(AXES, np.float32) * 3.5, size)
    assert face.tolist() == [0, 1, 2, 3, 4, 5] and valid.all()
    assert np.array_equal(idx, np.full((6, 2), (size - 1) / 2, np.float32))          # an axis hits the centre of its face
    face, idx, valid = cr.cube_indices(np.array([[1, 0.5, 0]], np.float32), size)     # +y is towards row 0
    assert face[0] == 0 and idx[0, 1] == np.float32((size - 1) / 2)
    assert idx[0, 0] == np.float32(max(0.25 * size - 0.5, 0)) and (size == 1 or idx[0, 0] < (size - 1) / 2)
    ties = {(1, 1, 1): 0, (-1, 1, 1): 1, (1, -1, -1): 0, (-1, -1, -1): 1, (1, 1, 0): 0, (0, 1, 1): 2, (-1, 0, 1): 1, (0, -1, 1): 3, (0, 0.5, -0.5): 2,
            (-1, 1, 0): 1, (0, 0, -2): 5, (1e-40, 0, 0): 0}
    d = np.array(list(ties), np.float32)
    face, idx, valid = cr.cube_indices(d, size)
    assert face.tolist() == list(ties.values()) and valid.all()
    assert np.array_equal(idx[0], [0, 0]) and np.array_equal(idx[1], [0, size - 1])   # (1, 1, 1): sc = -1, tc = -1; (-1, 1, 1): sc = +1
    bad = np.array([[0, 0, 0], [np.nan, 1, 0], [1, np.nan, 0], [0, 1, np.nan], [np.inf, 0, 0], [1, -np.inf, 0], [0, 0, np.inf], [-0., 0, -0.]], np.float32)
    face, idx, valid = cr.cube_indices(bad, size)
    assert not valid.any() and not face.any() and not idx.any()
    cube = np.arange(6 * size * size * 2, dtype=np.float32).reshape(6, size, size, 2) + 1
    assert not cr.sample(cube, bad).any() and not cr.sample(cube, bad, 'nearest').any()
    for dirs in (np.array(AXES, np.float32), d, bad):                                 # the torch form: the same three, exactly
        f_t, i_t, v_t = texture.directions_to_cube_indices(torch.from_numpy(dirs), size)
        f_r, i_r, v_r = cr.cube_indices(dirs, size)
        assert np.array_equal(f_t.numpy(), f_r) and np.array_equal(v_t.numpy(), v_r) and np.array_equal(i_t.numpy(), i_r)
        assert f_t.dtype == torch.int64 and i_t.dtype == torch.float32 and v_t.dtype == torch.bool


def test_each_face_is_oriented_as_opengl_lays_it_out():
    """A cube whose texel values are (face, row, col): 'nearest' at the direction built for a texel returns that texel, and the
    direction's components are the table's -- e.g. on +X the columns run towards -z and the rows towards -y."""
    size = 4
    cube = np.stack(np.meshgrid(np.arange(6), np.arange(size), np.arange(size), indexing='ij'), -1).astype(np.float32)
    f, r, c = (x.reshape(-1) for x in np.meshgrid(np.arange(6), np.arange(size), np.arange(size), indexing='ij'))
    d = dirs_from_indices(f, r, c, size, 2.0).astype(np.float32)
    assert np.array_equal(cr.sample(cube, d, 'nearest'), np.stack([f, r, c], -1).astype(np.float32))
    assert np.allclose(cr.sample(cube, d), np.stack([f, r, c], -1), rtol=0, atol=1e-5)         # texel centres: no blend
    x_face = d[(f == 0) & (r == 0)]
    assert (x_face[:, 0] == 2).all() and (np.diff(x_face[:, 2]) < 0).all() and (x_face[:, 1] > 0).all()


def _constructed_lookups(rng, n, size):
    """Look-ups away from every kink: the face, the texel and the fraction chosen first and inverted to a direction.  Fraction in
    [0.2, 0.8] and texel in [1, size - 3], so the unclamped index lies in (0.5, size - 1.5); size <= 17 keeps the second-largest
    component <= 0.8 a."""
    assert 4 <= size <= 17
    face = rng.integers(0, 6, n)
    row = rng.integers(1, size - 2, n) + rng.uniform(0.2, 0.8, n)
    col = rng.integers(1, size - 2, n) + rng.uniform(0.2, 0.8, n)
    d = dirs_from_indices(face, row, col, size, rng.uniform(0.5, 2.0, n))
    assert (np.sort(np.abs(d), -1)[:, 1] <= 0.8 * np.abs(d).max(-1)).all()
    lod = rng.integers(-1, 5, n) + rng.uniform(0.2, 0.8, n)      # with the bias below, lambda stays 0.1 from an integer
    return face, d.astype(np.float32), lod.astype(np.float32)


def test_reference_gradients_are_finite_differences():
    rng = np.random.default_rng(11)
    size, ct, n = 8, 3, 24
    cube = rng.uniform(-1, 1, (6, size, size, ct)).astype(np.float32)
    face, d, lod = _constructed_lookups(rng, n, size)
    assert np.array_equal(cr.Look(d).face, face)
    g = rng.standard_normal((n, ct))
    for filt, bias in (('bilinear', 0.0), ('trilinear', 0.0), ('trilinear', 0.0625)):
        l32 = lod if filt == 'trilinear' else None
        r = cr.grad(cube, d, g, filt, lod=l32, lod_bias=bias)

        def loss(c=cube, u=d, l=l32):
            return float((cr.sample(c, u, filt, lod=l, lod_bias=bias, dtype=np.float64) * g).sum())
        c64, d64 = cube.astype(np.float64), d.astype(np.float64)
        touched = np.argwhere(r['mass_cube'] > 0)
        for idx in [tuple(touched[k]) for k in rng.choice(len(touched), 6, replace=False)]:
            cp, cm = c64.copy(), c64.copy()
            cp[idx] += 1e-4; cm[idx] -= 1e-4
            fd = (loss(c=cp) - loss(c=cm)) / 2e-4
            assert abs(fd - r['grad_cube'][idx]) <= 1e-6 * max(1.0, r['mass_cube'][idx]), (filt, idx, fd, r['grad_cube'][idx])
        for idx in [(k, k % 3) for k in range(n)]:
            dp, dm = d64.copy(), d64.copy()
            dp[idx] += 1e-7; dm[idx] -= 1e-7
            fd = (loss(u=dp) - loss(u=dm)) / 2e-7
            assert abs(fd - r['grad_directions'][idx]) <= 1e-4 * max(1.0, r['mass_directions'][idx]), (filt, idx, fd, r['grad_directions'][idx])
        if filt == 'trilinear':
            l64 = lod.astype(np.float64)
            for idx in range(0, n, 2):
                lp, lm = l64.copy(), l64.copy()
                lp[idx] += 1e-6; lm[idx] -= 1e-6
                fd = (loss(l=lp) - loss(l=lm)) / 2e-6
                assert abs(fd - r['grad_lod'][idx]) <= 1e-5 * max(1.0, r['mass_lod'][idx]), (idx, fd, r['grad_lod'][idx])
            assert r['grad_lod'].any() and not r['grad_lod'][(lod + np.float32(bias) <= 0) | (lod + np.float32(bias) >= 3)].any()
        assert filt == 'trilinear' or r['grad_directions'].any(-1).all()


def test_direction_gradients_are_orthogonal_to_the_direction():
    rng = np.random.default_rng(12)
    cube = rng.uniform(-1, 1, (6, 8, 8, 2)).astype(np.float32)
    d = random_dirs(rng, (400,))
    g = rng.standard_normal((400, 2))
    lod = rng.uniform(-0.5, 3.5, 400).astype(np.float32)
    for filt in ('bilinear', 'trilinear'):
        r = cr.grad(cube, d, g, filt, lod=lod if filt == 'trilinear' else None)
        d64 = np.where(np.isfinite(d), d, 0).astype(np.float64)      # (an invalid direction: its gradient row is 0)
        dot, mass = np.abs((r['grad_directions'] * d64).sum(-1)), r['mass_directions'].sum(-1)
        assert (dot <= 1e-6 * mass * np.linalg.norm(d64, axis=-1)).all()
        assert (mass > 0).sum() > 300


@pytest.mark.parametrize('size,ct', [(1, 2), (5, 3), (8, 4)])
def test_torch_form_matches_the_reference(size, ct):
    """directions_to_cube_indices / sample_cube on the CPU: face and valid exactly, values to 2e-6 (the bound of
    tests/test_helpers_ref.py for ports), autograd against the reference's gradients at 1e-5 of their mass."""
    from dirt_amd import texture
    rng = np.random.default_rng(13 + size)
    cube = rng.uniform(-1, 1, (6, size, size, ct)).astype(np.float32)
    d = random_dirs(rng, (7, 30))
    g = rng.standard_normal((7, 30, ct)).astype(np.float32)
    for mode in ('bilinear', 'nearest'):
        c_t, d_t = torch.from_numpy(cube).requires_grad_(True), torch.from_numpy(d).requires_grad_(True)
        face, idx, valid = texture.directions_to_cube_indices(d_t, size)
        f_r, i_r, v_r = cr.cube_indices(d, size)
        assert np.array_equal(face.numpy(), f_r) and np.array_equal(valid.numpy(), v_r)
        assert np.allclose(idx.detach().numpy(), i_r, rtol=2e-6, atol=2e-6 * max(1.0, size))
        out = texture.sample_cube(c_t, face, idx, valid, mode)
        want = cr.sample(cube, d, mode)
        assert out.shape == want.shape and np.allclose(out.detach().numpy(), want, rtol=2e-6, atol=2e-6)
        gc, gd = torch.autograd.grad(out, [c_t, d_t], torch.from_numpy(g), allow_unused=True)
        r = cr.grad(cube, d, g, mode)
        _per_element(gc, r['grad_cube'], r['mass_cube'], 'torch %s grad_cube' % mode)
        _per_element(torch.zeros_like(d_t) if gd is None else gd, r['grad_directions'], r['mass_directions'], 'torch %s grad_directions' % mode)
        assert not out.detach().numpy()[~v_r].any()
    with pytest.raises(NotImplementedError):
        texture.sample_cube(c_t, face, idx, valid, 'trilinear')


def test_python_refusals_without_a_gpu():
    from dirt_amd import texture
    cube, d = torch.zeros(6, 4, 4, 3), torch.zeros(5, 7, 3)
    lod = torch.zeros(5, 7)

    def refused(text, *args, **kw):
        with pytest.raises(ValueError) as e:
            texture.sample_texture_cube(*args, **kw)
        assert str(e.value) == text, str(e.value)

    for bad in (torch.zeros(6, 4, 5, 3), torch.zeros(5, 4, 4, 3), torch.zeros(6, 4, 4), torch.zeros(6, 0, 0, 3), torch.zeros(6, 4, 4, 0)):
        refused('sample_texture_cube expects cube to be 4D [6, size, size, channels], got shape %s' % (tuple(bad.shape),), bad, d)
    for bad in (torch.zeros(5, 7, 2), torch.zeros(5, 4), torch.zeros(())):
        refused('sample_texture_cube expects directions of shape [..., 3], got %s' % (tuple(bad.shape),), cube, bad)
    refused('sample_texture_cube: cube must be a floating-point tensor, got torch.int32', cube.to(torch.int32), d)
    refused('sample_texture_cube: directions must be a floating-point tensor, got torch.int64', cube, d.to(torch.int64))
    refused('cube and directions must be on the same device (cpu vs meta)', cube, d.to('meta'))
    refused("sample_texture_cube: filter must be 'bilinear', 'nearest' or 'trilinear', got 'cubic'", cube, d, 'cubic')
    for filt in ('bilinear', 'nearest'):
        for kw in ({'lod': lod}, {'lod_bias': 0.5}, {'max_level': 1}):
            refused("lod, lod_bias and max_level apply to filter='trilinear' only (got filter=%r)" % filt, cube, d, filt, **kw)
    refused("sample_texture_cube: filter='trilinear' needs lod (a level of detail from the footprint of the directions is not supported)", cube, d, 'trilinear')
    refused('lod must be a tensor shaped like directions[..., 0] (5, 7), got (5, 6)', cube, d, 'trilinear', lod=torch.zeros(5, 6))
    refused('lod must be a tensor shaped like directions[..., 0] (5, 7), got ()', cube, d, 'trilinear', lod=1.0)
    refused('lod and directions must be on the same device (meta vs cpu)', cube, d, 'trilinear', lod=lod.to('meta'))
    refused('max_level must be a non-negative int or None, got -1', cube, d, 'trilinear', lod=lod, max_level=-1)
    for filt, kw in (('bilinear', {}), ('nearest', {}), ('trilinear', {'lod': lod})):
        with pytest.raises(RuntimeError) as e:
            texture.sample_texture_cube(cube, d, filt, **kw)
        assert str(e.value) == 'dirt_amd.texture.sample_texture_cube runs on an MI355X only; there is no CPU fallback'


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_the_library_declares_builds_and_exports_the_entry_points(lib):
    import dirt
    from dirt_amd import build, _lib
    header = open(os.path.join(ROOT, 'include', 'dirt_hip.h')).read()
    assert 'replace no reference interface' in header
    for symbol in (FWD, BWD):
        assert symbol in _lib.SYMBOLS and hasattr(lib, symbol) and re.search(r'\b%s\(' % symbol, header)
    assert 'dirt_texture_cube.hip' in build.SOURCES and 'dirt_texture_cube.hip' not in build.PER_SOURCE_FLAGS
    assert _lib.ABI_VERSION == 4
    assert dirt.texture.sample_texture_cube is __import__('dirt_amd').texture.sample_texture_cube and 'sample_texture_cube' in dirt.__doc__


def test_no_cube_kernel_uses_scratch_memory():
    from dirt_amd import build
    res = {k: v for k, v in build.kernel_resources().items() if 'texture_cube' in k}
    assert len(res) == 12, sorted(res)      # forward, backward, trilinear backward x channel counts 1, 3, 4, any
    assert all(v['scratch'] == 0 for v in res.values()), res


def test_c_abi_refusals_before_any_device_work(lib):
    """Every refusal of the two entry points, with pointers that are never dereferenced: the code, the whole message, and the
    rasteriser's error channel left as it was."""
    from dirt_amd import _lib
    one = ctypes.c_void_p(16)
    assert lib.dirt_workspace_bytes(-1, 3, 1, 16, 16, 3) == 0
    raster_text = lib.dirt_last_error()
    assert raster_text

    def fwd(pyr=one, dirs=one, lod=None, out=one, n=4, size=8, ch=3, levels=1, stride=3, bias=0.0, flags=0):
        return lib.dirt_texture_cube_forward(pyr, dirs, lod, out, n, size, ch, levels, stride, bias, flags, None)

    def bwd(pyr=one, dirs=one, lod=None, gout=one, gpyr=one, gdirs=one, glod=None, rows=2, cols=2, size=8, ch=3, levels=1, stride=3, gstride=3,
            bias=0.0, flags=0):
        return lib.dirt_texture_cube_backward(pyr, dirs, lod, gout, gpyr, gdirs, glod, rows, cols, size, ch, levels, stride, gstride, bias, flags, None)

    def refused(rc, text):
        assert rc == _lib.E_INVALID_ARGUMENT and lib.dirt_texture_last_error().decode() == text, lib.dirt_texture_last_error()
        assert lib.dirt_last_error() == raster_text

    for who, call in ((FWD, fwd), (BWD, bwd)):
        for flags in (_lib.TEX_CLAMP, _lib.TEX_CLAMP | _lib.TEX_NEAREST, 4):
            refused(call(flags=flags), '%s: flags 0x%x: a cube look-up takes DIRT_TEX_NEAREST only (its faces clamp to their edges)' % (who, flags))
        refused(call(flags=_lib.TEX_NEAREST, lod=one, levels=2), '%s: DIRT_TEX_NEAREST does not apply to a trilinear look-up (lod given)' % who)
        for kw in ({'size': 0}, {'size': -8}, {'ch': 0}, {'stride': 2}, {'stride': 0}):
            a = dict(size=8, ch=3, stride=3)
            a.update(kw)
            refused(call(**kw), '%s: bad sizes (n=4 size=%d channels=%d dir_stride=%d)' % (who, a['size'], a['ch'], a['stride']))
        for size, levels, most in ((8, 0, 4), (8, 5, 4), (12, 4, 3), (5, 2, 1), (1, 2, 1)):
            refused(call(size=size, levels=levels), '%s: %d levels, a %d x %d face has 1..%d' % (who, levels, size, size, most))
        for kw in ({'pyr': None}, {'dirs': None}):
            refused(call(**kw), '%s: pyramid / directions is NULL' % who)
    refused(fwd(n=-1), FWD + ': bad sizes (n=-1 size=8 channels=3 dir_stride=3)')
    refused(fwd(out=None), FWD + ': out is NULL')
    for kw in ({'gout': None}, {'gpyr': None}):
        refused(bwd(**kw), BWD + ': grad_out / grad_pyramid is NULL')
    refused(bwd(gstride=2), BWD + ': grad_dir_stride < 3')
    refused(bwd(glod=one), BWD + ': grad_lod needs lod')
    for rows, cols in ((-1, 2), (2, -1), (1 << 62, 4)):
        refused(bwd(rows=rows, cols=cols), BWD + ': bad pixel grid (rows=%d cols=%d)' % (rows, cols))
    for rows, cols in ((1, 1 << 31), (1 << 31, 2), (1 << 20, 1 << 40)):
        refused(bwd(rows=rows, cols=cols), BWD + ': pixel grid too large (rows=%d cols=%d)' % (rows, cols))
    # nothing to do is no error: no look-ups (every pointer may be NULL then)
    assert fwd(None, None, None, None, n=0) == 0 and lib.dirt_texture_last_error() == b''
    assert bwd(None, None, None, None, None, None, None, rows=0, cols=5) == 0 and lib.dirt_texture_last_error() == b''
    assert lib.dirt_last_error() == raster_text


# ---- the kernels against the restatement, on the GPU --------------------------------------------------------------------

def _per_element(got, want, mass, what, tol=TOL):
    got = (got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)).astype(np.float64)
    want, mass = np.asarray(want, np.float64), np.asarray(mass, np.float64)
    assert got.shape == want.shape == mass.shape, (what, got.shape, want.shape, mass.shape)
    assert np.isfinite(got).all(), what
    err, lim = np.abs(got - want), tol * mass + 1e-30
    if not np.all(err <= lim):
        worst = int(np.argmax(err - lim))
        raise AssertionError('%s: %d of %d elements outside %g * mass; worst err %g at mass %g (value %g)' % (
            what, int(np.sum(err > lim)), err.size, tol, err.flat[worst], mass.flat[worst], want.flat[worst]))


def _dev(gpu, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


def _check(gpu, cube, d, g, what, filt='bilinear', lod=None, want=('cube', 'directions', 'lod'), directions=None, **kw):
    """One fused look-up and its backward against the reference: the forward, and the gradients of the leaves in `want`; the others are
    not asked for and must come back as None.  `directions`: the tensor to pass (a view of something on the GPU that holds d)."""
    from dirt_amd import texture
    c_t = _dev(gpu, cube).requires_grad_('cube' in want)
    d_t = (_dev(gpu, d) if directions is None else directions.detach()).requires_grad_('directions' in want)
    l_t = _dev(gpu, lod).requires_grad_('lod' in want) if lod is not None else None
    out = texture.sample_texture_cube(c_t, d_t, filt, lod=l_t, **kw)
    ref_want, mag = cr.sample(cube, d, filt, lod=lod, magnitude=True, **kw)
    assert tuple(out.shape) == ref_want.shape
    if filt == 'nearest':
        assert np.array_equal(out.detach().cpu().numpy().view(np.uint32), ref_want.view(np.uint32)), what + ": 'nearest' is exact"
    else:
        _per_element(out, ref_want, mag, what + ' forward')
    assert not out.detach().cpu().numpy()[~cr.Look(d).valid.reshape(d.shape[:-1])].any()
    if not (out.requires_grad and want):
        return out
    out.backward(_dev(gpu, g))
    r = cr.grad(cube, d, g, filt, lod=lod, **kw)
    for name, leaf in (('cube', c_t), ('directions', d_t), ('lod', l_t)):
        if leaf is None:
            continue
        if name not in want:
            assert leaf.grad is None, (what, name)
            continue
        _per_element(leaf.grad, r['grad_' + name], r['mass_' + name], '%s grad_%s' % (what, name))
        if name != 'cube':   # an invalid look-up's rows: exactly zero
            bad = ~cr.Look(d).valid.reshape(d.shape[:-1])
            assert not leaf.grad.cpu().numpy()[bad].any(), (what, name)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 2, 3, 4, 5])
def test_sizes_channels_and_layouts(gpu, ct):
    rng = np.random.default_rng(200 + ct)
    for size in (1, 2, 5, 8):
        cube = rng.uniform(-1, 1, (6, size, size, ct)).astype(np.float32)
        for shape in ((19, 35), (300,), (2, 17, 16)):
            d = random_dirs(rng, shape)
            g = rng.standard_normal(shape + (ct,)).astype(np.float32)
            for filt in ('bilinear', 'nearest'):
                _check(gpu, cube, d, g, 'N=%d C=%d %s %s' % (size, ct, shape, filt), filt)
    # read in place from gbuffer[..., 4:7] of a [H, W, 10] G-buffer (the gradient lands in those channels only), and from a
    # non-contiguous tensor, which is copied
    cube = rng.uniform(-1, 1, (6, 5, 5, ct)).astype(np.float32)
    d = random_dirs(rng, (19, 35))
    g = rng.standard_normal((19, 35, ct)).astype(np.float32)
    gbuf = rng.standard_normal((19, 35, 10)).astype(np.float32)
    gbuf[..., 4:7] = d
    from dirt_amd import texture, _stage
    gb = _dev(gpu, gbuf).requires_grad_(True)
    assert _stage.rows_in_place(gb[..., 4:7], 3)[1] == 10
    out = texture.sample_texture_cube(_dev(gpu, cube), gb[..., 4:7])
    out.backward(_dev(gpu, g))
    r = cr.grad(cube, d, g)
    _per_element(out, *cr.sample(cube, d, magnitude=True), 'in place forward')
    _per_element(gb.grad[..., 4:7], r['grad_directions'], r['mass_directions'], 'in place grad_directions')
    assert not gb.grad[..., :4].any() and not gb.grad[..., 7:].any()
    turned = _dev(gpu, d.transpose(1, 0, 2)).transpose(0, 1)
    assert not turned.is_contiguous()
    _check(gpu, cube, d, g, 'non-contiguous', directions=turned)


@pytest.mark.gpu
def test_every_pattern_of_wanted_gradients(gpu):
    rng = np.random.default_rng(210)
    cube = rng.uniform(-1, 1, (6, 8, 8, 3)).astype(np.float32)
    d = random_dirs(rng, (21, 18))
    g = rng.standard_normal((21, 18, 3)).astype(np.float32)
    lod = rng.uniform(-0.5, 3.5, (21, 18)).astype(np.float32)
    for want in (('cube',), ('directions',), ('cube', 'directions')):
        for filt in ('bilinear', 'nearest'):
            _check(gpu, cube, d, g, '%s %s' % (filt, want), filt, want=want)
    for want in (('cube',), ('directions',), ('lod',), ('cube', 'directions'), ('cube', 'lod'), ('directions', 'lod'), ('cube', 'directions', 'lod')):
        _check(gpu, cube, d, g, 'trilinear %s' % (want,), 'trilinear', lod=lod, want=want)
    out = _check(gpu, cube, d, g, 'no gradient', want=())
    assert not out.requires_grad


def _tile_scene(rng):
    """A 48 x 80 image of directions into a cube of 64: fifteen 16 x 16 tiles, one per case.  -> (directions, {tile: name})"""
    size, H, W = 64, 48, 80
    py, px = np.meshgrid(np.arange(16.), np.arange(16.), indexing='ij')
    d = np.zeros((H, W, 3), np.float32)

    def put(ty, tx, block):
        d[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] = block

    def spread(face, r0, rows, c0, cols):   # taps from texel r0 to r0 + rows - 1, c0 to c0 + cols - 1
        return dirs_from_indices(face, r0 + 0.5 + py * (rows - 2) / 15., c0 + 0.5 + px * (cols - 2) / 15., size, 1.5)

    put(0, 0, spread(2, 10, 6, 20, 7))                 # a small box on one face
    put(0, 1, spread(5, 3, 40, 20, 40))                # exactly TEX_PATCH texels: the patch
    put(0, 2, spread(1, 3, 41, 20, 40))                # one row more: direct
    put(0, 3, dirs_from_indices(0, 30 + py, 60 + px * 0.23, size))  # columns 60 .. 63.45: the last ones past texel 63's centre, clamped to it
    edge = np.stack([1 + 0.02 * (px - 7.5), 0.3 + 0.01 * py, 1 + 0.0 * px], -1)      # x ~ z: +X and +Z
    put(0, 4, edge)
    corner = np.ones((16, 16, 3)) + 0.05 * rng.uniform(-1, 1, (16, 16, 3))            # around (1, 1, 1): +X, +Y, +Z
    put(1, 0, corner)
    put(1, 1, np.zeros((16, 16, 3)))                   # only invalid look-ups
    holes = spread(3, 40, 9, 8, 9)                     # invalid look-ups scattered in a valid tile
    holes[rng.uniform(0, 1, (16, 16)) < 0.2] = [[np.nan, 1, 1]]
    holes[5, 5] = 0
    holes[9, 2] = [1, -np.inf, 0]
    put(1, 2, holes)
    put(1, 3, -corner)                                 # the opposite corner
    put(1, 4, spread(4, 0, 3, 61, 3))
    for tx in range(5):                                # a row of random directions: every face in every tile, some invalid
        put(2, tx, random_dirs(rng, (16, 16)))
    return d


def _tile_classes(d, size, patch=1600):
    """From the reference's taps: per 16 x 16 tile (faces touched, box height, box width), None for a tile without valid look-ups."""
    valid, face, r0, r1, c0, c1 = (x.reshape(d.shape[:-1]) for x in cr.level0_taps(d, size))
    out = {}
    for ty in range(d.shape[0] // 16):
        for tx in range(d.shape[1] // 16):
            s = (slice(16 * ty, 16 * ty + 16), slice(16 * tx, 16 * tx + 16))
            v = valid[s]
            if not v.any():
                out[ty, tx] = None
                continue
            out[ty, tx] = (len(set(face[s][v])), int(r1[s][v].max() - r0[s][v].min() + 1), int(c1[s][v].max() - c0[s][v].min() + 1), int((~v).sum()))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 6])
def test_backward_tile_classes_and_invalid_lookups(gpu, ct):
    """Every class of backward tile in one image (worked out from the reference's taps, not by instrumenting the kernel): a
    small box on one face, a box of exactly 40 x 40 texels (the LDS patch), 41 x 40 (direct), a tile over a face edge, tiles
    over a cube corner (three faces), a tile of invalid look-ups only and one with invalid look-ups among valid ones."""
    rng = np.random.default_rng(220)
    size = 64
    d = _tile_scene(rng)
    classes = _tile_classes(d, size)
    assert classes[0, 0][:3] == (1, 6, 7) and classes[0, 1][:3] == (1, 40, 40) and classes[0, 2][:3] == (1, 41, 40)
    assert classes[0, 3][0] == 1 and classes[0, 4][0] == 2 and classes[1, 0][0] == 3 and classes[1, 3][0] == 3
    assert classes[1, 1] is None and classes[1, 2][0] == 1 and 20 < classes[1, 2][3] < 100 and classes[1, 2][1] * classes[1, 2][2] <= 1600
    assert all(classes[2, tx][0] >= 4 for tx in range(5))
    cube = rng.uniform(-1, 1, (6, size, size, ct)).astype(np.float32)
    g = rng.standard_normal(d.shape[:-1] + (ct,)).astype(np.float32)
    for filt in ('bilinear', 'nearest'):
        _check(gpu, cube, d, g, 'tiles C=%d %s' % (ct, filt), filt)
    _check(gpu, cube, d.reshape(-1, 3), g.reshape(-1, ct), 'tiles as a flat list C=%d' % ct)       # 256 x 1 tiles


@pytest.mark.gpu
def test_ties_and_corners_pick_the_reference_face(gpu):
    from dirt_amd import texture
    rng = np.random.default_rng(230)
    signs = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], np.float32)
    d = np.concatenate([signs * s for s in (1.0, 0.3, 7.0)] + [signs * rng.uniform(0.5, 2, (27, 1)).astype(np.float32),
                       random_dirs(rng, (200,)), np.array([[1, 1, np.nextafter(np.float32(1), np.float32(2))], [1e-40, 1e-41, 0], [-2e-45, 0, 1e-45]], np.float32)])
    cube = np.broadcast_to(np.arange(1, 7, dtype=np.float32)[:, None, None, None], (6, 4, 4, 1)).copy()   # six distinct constants
    q = cr.Look(d)
    want = np.where(q.valid, q.face + 1, 0).astype(np.float32)
    assert set(want.tolist()) == {0, 1, 2, 3, 4, 5, 6}
    for filt in ('bilinear', 'nearest'):
        got = texture.sample_texture_cube(_dev(gpu, cube), _dev(gpu, d), filt)[:, 0].cpu().numpy()
        if filt == 'bilinear':   # four weights that sum to 1 within an ulp or two: the face's constant to that, never another face's
            assert np.abs(got - want).max() <= TOL * 6
            got = np.rint(got)
        assert np.array_equal(got, want), (filt, d[got != want], got[got != want], want[got != want])


@pytest.mark.gpu
@pytest.mark.parametrize('filt', ['bilinear', 'nearest', 'trilinear'])
def test_c_abi_writes_inside_its_outputs_only(gpu, lib, filt):
    """Sentinels before and after out, grad_directions (stride 5: the two floats between rows too) and grad_lod stay; grad_pyramid,
    handed over full of garbage, comes back as the gradient alone; no look-ups still clears it."""
    from dirt_amd import _lib, rasterise_ops as ops, texture
    rng = np.random.default_rng(240)
    size, ct, n, pad = 8, 3, 333, 7
    cube = rng.uniform(-1, 1, (6, size, size, ct)).astype(np.float32)
    d = random_dirs(rng, (n,))
    g = rng.standard_normal((n, ct)).astype(np.float32)
    lod = rng.uniform(-0.5, 3.5, n).astype(np.float32) if filt == 'trilinear' else None
    levels = 4 if filt == 'trilinear' else 1
    pyr = torch.stack([torch.cat([lv.reshape(-1) for lv in texture.mip_pyramid(_dev(gpu, cube[f]))]) for f in range(6)]) if levels > 1 else _dev(gpu, cube).reshape(6, -1)
    floats = pyr.shape[1]
    flags = _lib.TEX_NEAREST if filt == 'nearest' else 0
    stream = ops._stream_handle(gpu)
    out = torch.full((pad + n * ct + pad,), SENTINEL, device=gpu)
    d_t, g_t, l_t = _dev(gpu, d), _dev(gpu, g), _dev(gpu, lod) if lod is not None else None
    lp = l_t.data_ptr() if l_t is not None else None
    assert lib.dirt_texture_cube_forward(pyr.data_ptr(), d_t.data_ptr(), lp, out.data_ptr() + 4 * pad, n, size, ct, levels, 3, 0.0, flags, stream) == 0
    gpyr = torch.full((pad + 6 * floats + pad,), SENTINEL, device=gpu)
    gpyr[pad:-pad] = float('nan')
    gpyr[pad:-pad:3] = 1e30
    gdirs = torch.full((pad + n * 5 + pad,), SENTINEL, device=gpu)
    glod = torch.full((pad + n + pad,), SENTINEL, device=gpu)
    assert lib.dirt_texture_cube_backward(pyr.data_ptr(), d_t.data_ptr(), lp, g_t.data_ptr(), gpyr.data_ptr() + 4 * pad, gdirs.data_ptr() + 4 * pad,
                                          glod.data_ptr() + 4 * pad if lod is not None else None, 1, n, size, ct, levels, 3, 5, 0.0, flags, stream) == 0
    torch.cuda.synchronize()
    want, mag = cr.sample(cube, d, filt, lod=lod, magnitude=True)
    r = cr.grad(cube, d, g, filt, lod=lod)
    assert (out[:pad] == SENTINEL).all() and (out[-pad:] == SENTINEL).all()
    _per_element(out[pad:-pad].view(n, ct), want, mag, 'forward')
    assert (gpyr[:pad] == SENTINEL).all() and (gpyr[-pad:] == SENTINEL).all()
    got = gpyr[pad:-pad].view(6, floats)
    if levels > 1:
        collapsed = torch.empty(6, size, size, ct, device=gpu)
        assert lib.dirt_texture_mip_collapse_batch(got.contiguous().data_ptr(), collapsed.data_ptr(), 6, size, size, ct, levels, stream) == 0
        torch.cuda.synchronize()
        got = collapsed
    _per_element(got.reshape(6, size, size, ct), r['grad_cube'], r['mass_cube'], 'grad_pyramid')
    rows = gdirs[pad:-pad].view(n, 5)
    assert (gdirs[:pad] == SENTINEL).all() and (gdirs[-pad:] == SENTINEL).all() and (rows[:, 3:] == SENTINEL).all()
    _per_element(rows[:, :3], r['grad_directions'], r['mass_directions'], 'grad_directions')
    if lod is not None:
        assert (glod[:pad] == SENTINEL).all() and (glod[-pad:] == SENTINEL).all()
        _per_element(glod[pad:-pad], r['grad_lod'], r['mass_lod'], 'grad_lod')
    else:
        assert (glod == SENTINEL).all()
    # no look-ups: the gradient is cleared all the same, and nothing else is touched
    gpyr.fill_(3.0)
    assert lib.dirt_texture_cube_backward(pyr.data_ptr(), None, None, None, gpyr.data_ptr() + 4 * pad, None, None, 0, 9, size, ct, levels, 3, 3, 0.0, flags, stream) == 0
    torch.cuda.synchronize()
    assert (gpyr[:pad] == 3).all() and (gpyr[-pad:] == 3).all() and not gpyr[pad:-pad].any()


@pytest.mark.gpu
@pytest.mark.parametrize('size,levels', [(8, 4), (12, 3)])
@pytest.mark.parametrize('ct', [1, 3, 4, 5])
def test_trilinear(gpu, size, levels, ct):
    assert mr.level_count(size, size) == levels
    rng = np.random.default_rng(250 + size + ct)
    cube = rng.uniform(-1, 1, (6, size, size, ct)).astype(np.float32)
    d = random_dirs(rng, (23, 37))
    g = rng.standard_normal((23, 37, ct)).astype(np.float32)
    lod = rng.uniform(-1, levels, (23, 37)).astype(np.float32)
    lod[0, :8] = [-0.5, 0.0, 1.0, 2.0, levels - 1, levels + 0.5, np.nan, 0.5]
    lod[1, :levels] = np.arange(levels)
    _check(gpu, cube, d, g, 'trilinear N=%d C=%d' % (size, ct), 'trilinear', lod=lod)
    _check(gpu, cube, d, g, 'trilinear N=%d C=%d bias' % (size, ct), 'trilinear', lod=lod, lod_bias=-0.375)
    _check(gpu, cube, d, g, 'trilinear N=%d C=%d max_level' % (size, ct), 'trilinear', lod=lod, lod_bias=0.25, max_level=1)
    _check(gpu, cube, d.reshape(-1, 3)[:300], g.reshape(-1, ct)[:300], 'trilinear N=%d C=%d flat' % (size, ct), 'trilinear', lod=lod.reshape(-1)[:300])


def _trilinear_tile_classes(d, lod, size, levels):
    """From the reference's level split and taps: per 16 x 16 tile (faces touched, levels spanned, texels of the two levels' tap
    boxes together -- None where the tile has several faces or more than two levels), None for a tile without valid look-ups."""
    q = cr.Look(d)
    shape = d.shape[:-1]
    valid, face = q.valid.reshape(shape), q.face.reshape(shape)
    lev, f = mr._split(lod.astype(np.float32), levels, np.float32)
    top = lev + (f != 0)
    boxes = []
    for k in range(levels):
        n = max(size >> k, 1)
        row, col = cr.index(q.t, n)[0], cr.index(q.s, n)[0]
        boxes.append([x.reshape(shape) for x in mr._taps(row, col, n, n, np.float32)[:4]])
    out = {}
    for ty in range(shape[0] // 16):
        for tx in range(shape[1] // 16):
            s = (slice(16 * ty, 16 * ty + 16), slice(16 * tx, 16 * tx + 16))
            v = valid[s]
            if not v.any():
                out[ty, tx] = None
                continue
            faces, lmin, lmax = len(set(face[s][v])), int(lev[s][v].min()), int(top[s][v].max())
            used = None
            if faces == 1 and lmax - lmin <= 1:
                used = 0
                for k in range(lmin, lmax + 1):
                    on = v & ((lev[s] == k) | ((top[s] == k) & (f[s] != 0)))
                    r0, r1, c0, c1 = (b[s][on] for b in boxes[k])
                    used += int((r1.max() - r0.min() + 1) * (c1.max() - c0.min() + 1)) if on.any() else 0
            out[ty, tx] = (faces, lmax - lmin + 1, used)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 6])
def test_trilinear_backward_tile_classes(gpu, ct):
    """The trilinear backward's classes of tile, worked out from the reference: one face and one level, one face and two adjacent
    levels whose boxes fit the LDS patch together, the same with boxes that do not fit, more than two levels, several faces, and
    a tile of invalid look-ups only."""
    rng = np.random.default_rng(225)
    size, levels = 64, 7
    d = _tile_scene(rng)
    lod = np.zeros(d.shape[:-1], np.float32)
    px = np.broadcast_to(np.arange(16, dtype=np.float32), (16, 16))
    for (ty, tx), value in {(0, 0): 0.5, (0, 1): 0.5, (0, 2): 2.5 + 0.02 * px, (0, 3): 1.0, (0, 4): 1.5, (1, 0): 0.75, (1, 2): 1.25 + 0.04 * px,
                            (1, 3): 3.5, (1, 4): 0.2 + 0.24 * px}.items():
        lod[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] = value
    lod[32:] = rng.uniform(-1, levels, (16, 80))
    lod[40, :5] = [np.nan, 6.0, 6.5, -0.0, 5.0]
    classes = _trilinear_tile_classes(d, lod, size, levels)
    assert classes[0, 0] == (1, 2, 6 * 7 + 4 * 4) and classes[0, 1][:2] == (1, 2) and classes[0, 1][2] > 1600
    assert classes[0, 2][:2] == (1, 2) and classes[0, 2][2] <= 1600 and classes[0, 3][:2] == (1, 1) and classes[0, 3][2] <= 1600
    assert classes[0, 4][0] == 2 and classes[1, 0][0] == 3 and classes[1, 1] is None and classes[1, 3][0] == 3
    assert classes[1, 2][:2] == (1, 2) and classes[1, 2][2] <= 1600 and classes[1, 4][:2] == (1, 5)
    cube = rng.uniform(-1, 1, (6, size, size, ct)).astype(np.float32)
    g = rng.standard_normal(d.shape[:-1] + (ct,)).astype(np.float32)
    _check(gpu, cube, d, g, 'trilinear tiles C=%d' % ct, 'trilinear', lod=lod)
    _check(gpu, cube, d.reshape(-1, 3), g.reshape(-1, ct), 'trilinear tiles as a flat list C=%d' % ct, 'trilinear', lod=lod.reshape(-1), lod_bias=0.125)


@pytest.mark.gpu
def test_trilinear_on_a_cube_of_one_level_and_at_lod_zero(gpu):
    """N = 5 has one level: every lod gives the bilinear look-up, bit for bit, as lod <= 0 does on any cube."""
    from dirt_amd import texture
    rng = np.random.default_rng(260)
    d = _dev(gpu, random_dirs(rng, (40, 33)))
    for size in (5, 8):
        cube = _dev(gpu, rng.uniform(-1, 1, (6, size, size, 3)).astype(np.float32))
        lod = torch.rand(40, 33, device=gpu) * 4 - 1 if size == 5 else -torch.rand(40, 33, device=gpu)
        tri = texture.sample_texture_cube(cube, d, 'trilinear', lod=lod)
        assert torch.equal(tri.view(torch.int32), texture.sample_texture_cube(cube, d).view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize('filt', ['bilinear', 'trilinear'])
def test_backward_twice_does_not_accumulate(gpu, filt):
    from dirt_amd import texture
    rng = np.random.default_rng(270)
    cube, d = rng.uniform(-1, 1, (6, 8, 8, 3)).astype(np.float32), random_dirs(rng, (30, 40))
    g = rng.standard_normal((30, 40, 3)).astype(np.float32)
    lod = rng.uniform(-0.5, 3.5, (30, 40)).astype(np.float32) if filt == 'trilinear' else None
    leaves = [_dev(gpu, cube).requires_grad_(True), _dev(gpu, d).requires_grad_(True)] + ([_dev(gpu, lod).requires_grad_(True)] if lod is not None else [])
    out = texture.sample_texture_cube(leaves[0], leaves[1], filt, lod=leaves[2] if lod is not None else None)
    first = torch.autograd.grad(out, leaves, _dev(gpu, g), retain_graph=True)
    second = torch.autograd.grad(out, leaves, _dev(gpu, g), retain_graph=True)
    r = cr.grad(cube, d, g, filt, lod=lod)
    for name, a, b in zip(('cube', 'directions', 'lod'), first, second):
        _per_element(a, r['grad_' + name], r['mass_' + name], 'first grad_' + name)
        _per_element(b, a.cpu().numpy(), r['mass_' + name], 'second grad_' + name)


@pytest.mark.gpu
@pytest.mark.parametrize('filt', ['bilinear', 'trilinear'])
def test_a_captured_lookup_and_backward_replay_on_a_new_cube(gpu, filt):
    """No host synchronisation in the look-up or its backward: captured with torch.cuda.graph on one stream and replayed after the
    cube was rewritten in place, the replay matches the reference for the new contents (the clear of the gradient included: face
    -Z is touched by no look-up and comes back 0)."""
    from dirt_amd import texture
    rng = np.random.default_rng(280)
    cube = rng.uniform(-1, 1, (6, 8, 8, 3)).astype(np.float32)
    d = random_dirs(rng, (24, 40))
    d[(np.abs(d[..., 2]) >= np.abs(d[..., 0])) & (np.abs(d[..., 2]) >= np.abs(d[..., 1])) & (d[..., 2] < 0)] *= -1     # nothing on -Z
    g = rng.standard_normal((24, 40, 3)).astype(np.float32)
    lod = rng.uniform(-0.5, 3.5, (24, 40)).astype(np.float32) if filt == 'trilinear' else None
    c_t, d_t, g_t = _dev(gpu, cube), _dev(gpu, d), _dev(gpu, g)
    l_t = _dev(gpu, lod) if lod is not None else None

    def step():
        leaves = [x.detach().requires_grad_(True) for x in (c_t, d_t)]
        out = texture.sample_texture_cube(leaves[0], leaves[1], filt, lod=l_t)
        return (out.detach(),) + tuple(torch.autograd.grad(out, leaves, g_t))

    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g, gc_g, gd_g = step()
    for k in range(2):
        cube_k = rng.uniform(-1, 1, cube.shape).astype(np.float32)
        with torch.no_grad():
            c_t.copy_(_dev(gpu, cube_k))
        graph.replay()
        torch.cuda.synchronize()
        _per_element(out_g, *cr.sample(cube_k, d, filt, lod=lod, magnitude=True), 'replay %d forward' % k)
        r = cr.grad(cube_k, d, g, filt, lod=lod)
        _per_element(gc_g, r['grad_cube'], r['mass_cube'], 'replay %d grad_cube' % k)
        _per_element(gd_g, r['grad_directions'], r['mass_directions'], 'replay %d grad_directions' % k)
        assert not r['mass_cube'][5].any() and not gc_g[5].any()


@pytest.mark.gpu
def test_end_to_end_rasterise_deferred_with_a_cube_map_shader(gpu):
    """rasterise_deferred at 32 x 32 over a small mesh with a shader that looks the interpolated normals up in a cube (the
    background's normals are (0, 0, 0): black without a mask), against the same shader written with the pure-torch form.
    The G-buffer is the same in both runs, so the reference (tests/cube_reference.py) at the normals the shader saw gives each
    pixel's magnitude and each gradient's L1 mass: pixels, the gradient to the cube and the gradient that leaves the shader for
    the normals are compared per element at TOL of those.  The vertex gradient is the rasteriser's backward of that normal
    gradient and of the shaded pixels (the filtered image), the same map in both runs, linear in the former; its per-element mass
    is not available without the map's absolute values, so it is held to TOL of the L1 norm of the torch form's vertex
    gradient, a lower bound of the summed masses."""
    import dirt_amd as dirt
    from dirt_amd import lighting, matrices, texture
    rng = np.random.default_rng(290)
    v = np.array([[-1, -1, 0.2], [1, -1, -0.3], [1, 1, 0.4], [-1, 1, -0.1], [0, 0, 1.0]], np.float32) * 0.8
    faces = _dev(gpu, np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], np.int32))
    cube = rng.uniform(-1, 1, (6, 8, 8, 3)).astype(np.float32)
    g = rng.standard_normal((32, 32, 3)).astype(np.float32)
    seen = {}

    def render(fused):
        vertices, c_t = _dev(gpu, v).requires_grad_(True), _dev(gpu, cube).requires_grad_(True)
        view = matrices.translation(torch.tensor([0., 0., -3.], device=gpu))
        projection = matrices.perspective_projection(near=0.1, far=20., right=0.05, aspect=1.).to(gpu)
        clip = (torch.cat([vertices, torch.ones_like(vertices[:, :1])], dim=1) @ view) @ projection
        attributes = torch.cat([torch.ones_like(vertices[:, :1]), lighting.vertex_normals(vertices, faces)], dim=1)

        def shader_fn(gbuffer, env):
            normals = gbuffer[..., 1:4]
            seen[fused] = normals.detach().cpu().numpy()
            if normals.requires_grad:
                normals.register_hook(lambda grad: seen.__setitem__((fused, 'grad'), grad.detach().cpu().numpy()))
            if fused:
                return texture.sample_texture_cube(env, normals)
            return texture.sample_cube(env, *texture.directions_to_cube_indices(normals, env.shape[1]))

        pixels = dirt.rasterise_deferred(background_attributes=torch.zeros([32, 32, 4], device=gpu), vertices=clip, vertex_attributes=attributes,
                                         faces=faces, shader_fn=shader_fn, shader_additional_inputs=[c_t])
        gc, gv = torch.autograd.grad(pixels, [c_t, vertices], _dev(gpu, g))
        return pixels.detach(), gc, gv

    (p_f, gc_f, gv_f), (p_t, gc_t, gv_t) = render(True), render(False)
    normals = seen[True].reshape(32, 32, 3)
    assert np.array_equal(normals, seen[False].reshape(32, 32, 3))
    covered = float(cr.Look(normals).valid.mean())
    assert 0.2 < covered < 0.9, covered
    want, mag = cr.sample(cube, normals, magnitude=True)
    r = cr.grad(cube, normals, g)
    assert tuple(p_f.shape) == (32, 32, 3)
    for name, (pixels, gc, gv) in (('fused', (p_f, gc_f, gv_f)), ('torch form', (p_t, gc_t, gv_t))):
        _per_element(pixels, want, mag, name + ' pixels')
        _per_element(gc, r['grad_cube'], r['mass_cube'], name + ' grad_cube')
        _per_element(seen[name == 'fused', 'grad'].reshape(32, 32, 3), r['grad_directions'], r['mass_directions'], name + ' grad of the normals')
    assert (p_f - p_t).abs().max().item() <= 2 * TOL * float(mag.max())
    norm = gv_t.abs().sum().item()
    assert norm > 0 and (gv_f - gv_t).abs().max().item() <= TOL * norm, ((gv_f - gv_t).abs().max().item(), norm)


