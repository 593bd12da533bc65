"""`shading.environment_background` (dirt_background.hip) where tests/test_background.py stops: images of one row (the scatter's
grid becomes 1 x (scenes x cols)), alone, with the footprint and as a batch; more rows of partial sums than one turn of the
reductions of d matrix and d intensity takes, of one scene and of three scenes into one shared sum; a cube whose faces are
larger than the LDS patch; a NaN in the matrix, in the mask and in the environment and a mask value outside [0, 1]; the C ABI
on a batch of one-row images and on an empty call.

The method is tests/test_background.py's, and so are `make`, `camera` and `masks`: tests/background_reference.py is the float64
reference, the float32 torch form's worst |f32 - ref64| / mass per kind of result over THIS file's cases is the F32 table below
(`python -m tests.test_background_edges` prints it; `measure` makes it, with HEADROOM for the order of the torch form's own
sums), the kernel gets KERNEL times that, an element of zero mass must be exact, pixels on kinks are left out as there and no case leaves out more than a tenth.  The table is this file's
own: growing the old one would loosen the old tests.  Each designed case has a test without a GPU that it stands where it is
meant to."""
import functools

import numpy as np
import pytest
import torch

from tests import background_reference as R
from tests.test_background import KERNEL, ROTATIONS, TEX_PATCH, TILE, _dev, camera, make, masks, run_kernel

# python -m tests.test_background_edges
F32 = {'out': 7.15e-5, 'd_environment': 7.15e-4, 'd_matrix': 2.95e-7, 'd_intensity': 5.88e-7, 'd_mask': 1.72e-5}
HEADROOM = 1.1      # on the measured figures: the torch form adds its float32 sums in an order that depends on the machine's threads
ROW = (1, 300)      # tiles of 256 x 1: one full, one of 44 pixels
BAD = (17, 19)
NAN_PIXEL, TWO_PIXEL = (5, 7), (11, 3)
NAN_TEXEL = (4, 6, 5, 1)      # face, row, column, channel of a 12 x 12 cube


def batch(seed, size, matrices, mask, intensity, **kw):
    """B = 3 scenes of `size`; `matrices`, `mask`, `intensity`: 'shared' or 'scene' (`batch_case` of tests/test_background.py at
    any size)"""
    rng = np.random.default_rng(seed)
    M = np.stack([camera(ROTATIONS[b], size) for b in range(3)]) if matrices == 'scene' else camera(ROTATIONS[3], size)
    m = np.stack([masks(k, size, rng) for k in ('mixed', 'fraction', 'zero')]) if mask == 'scene' else masks('mixed', size, rng)
    I = rng.uniform(-1., 1., (3, 3)) if intensity == 'scene' else (0.7, 1.1, -0.4)
    return make(seed, size, M=M, mask=m, intensity=I, **kw)


def poisoned_mask(pixel, value):
    m = masks('fraction', BAD, np.random.default_rng(440))
    m[pixel] = value
    return m


@functools.lru_cache(maxsize=None)
def case(name):
    if name == 'row':
        return make(400, ROW, rotation=1)
    if name == 'row-footprint':
        return make(401, ROW, n=96, filter='trilinear', lod=None, lod_bias=0.9, rotation=1)      # a thin image's footprint is small: lambda -1 .. 0.9
    if name == 'row-batch':
        return batch(402, ROW, 'scene', 'scene', 'scene')
    if name == 'tiles-260':                       # 2 x 130 tiles
        return make(410, (17, 2065), rotation=2)
    if name == 'tiles-261':                       # 3 scenes of 3 x 29 tiles into one sum of d matrix and one of d intensity
        return batch(411, (33, 464), 'shared', 'scene', 'shared')
    if name == 'n64':                             # a face of 4096 texels
        return make(420, (33, 35), n=64, rotation=5)
    if name == 'n64-lod':
        return make(421, (33, 35), n=64, filter='trilinear', lod=0.6, rotation=5)
    if name == 'nan-matrix':
        M = camera(ROTATIONS[1], BAD)
        M[1, 2] = np.nan
        return make(430, BAD, M=M)
    if name == 'nan-mask':
        return make(431, BAD, rotation=1, mask=poisoned_mask(NAN_PIXEL, np.nan))
    if name == 'mask-two':
        return make(432, BAD, rotation=1, mask=poisoned_mask(TWO_PIXEL, 2.))
    if name == 'nan-texel':
        cube = np.random.default_rng(433).standard_normal((6, 12, 12, 3)).astype(np.float32)
        cube[NAN_TEXEL] = np.nan
        return make(433, BAD, rotation=1, levels=[cube])
    raise KeyError(name)


ROWS_ONE = ['row', 'row-footprint', 'row-batch']
MANY_TILES = ['tiles-260', 'tiles-261']
LARGE = ['n64', 'n64-lod']
FINITE = ROWS_ONE + MANY_TILES + LARGE + ['nan-matrix', 'mask-two']
WITH_NANS = ['nan-mask', 'nan-texel']


def measure():
    """-> the table: the float32 torch form's worst ratio per kind of result over this file's cases (a NaN of the reference has
    no mass and is not compared), and per case its figures"""
    table, rows = dict.fromkeys(R.KINDS, 0.), []
    for name in FINITE + WITH_NANS:
        c = case(name)
        args, kw = c.args
        worst = R.ratios(R.torch_form(*args, operand=c.operand, **kw), c.ref, c.operand)
        rows.append((name, c.share, worst))
        for k, v in worst.items():
            assert v == v, (name, k)
            table[k] = max(table[k], v)
    return {k: float('%.2e' % (v * HEADROOM)) for k, v in table.items()}, rows


def same_nans(got, c):
    """the NaN of every kind of result are the restatement's: of the per-pixel kinds on the compared pixels, of the sums all"""
    ref = c.ref
    want_env, _ = R.environment_grad(ref, c.operand)
    for kind, want, keep in (('out', ref['out'], c.keep), ('d_mask', ref['d_mask'], c.keep), ('d_matrix', ref['d_matrix'], None),
                             ('d_intensity', ref['d_intensity'], None), ('d_environment', want_env, None)):
        x = np.asarray(got[kind]).reshape(want.shape)
        a, b = (np.isnan(x), np.isnan(want)) if keep is None else (np.isnan(x)[keep], np.isnan(want)[keep])
        assert np.array_equal(a, b), (kind, int(a.sum()), int(b.sum()))
        assert not np.isinf(x).any(), kind


# ---- without a GPU

def test_no_case_leaves_out_more_than_a_tenth():
    for name in FINITE + WITH_NANS:
        assert case(name).share <= 0.10, (name, case(name).share)


@pytest.mark.parametrize('name', FINITE + WITH_NANS)
def test_the_float32_torch_form_against_the_restatement(name):
    """Per element, relative to the element's mass: within this file's F32 table, whose figures are this test's own worst ones;
    where the restatement holds a NaN, so does the torch form, and nowhere else"""
    c = case(name)
    args, kw = c.args
    got = R.torch_form(*args, operand=c.operand, **kw)
    worst = R.ratios(got, c.ref, c.operand)
    print(name, {k: '%.2e' % v for k, v in worst.items()})
    for kind, x in worst.items():
        assert x <= F32[kind], (kind, x)
    if name in WITH_NANS:
        same_nans(got, c)
    else:
        assert R.exact_where_massless(got, c.ref, c.operand)
        assert all(np.isfinite(np.asarray(v)).all() for v in got.values() if v is not None)


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import _lib
    return _lib.load()


def tiles_of(lib, c):
    """the tiles of one scene's image, from the scratch the library asks for: a row of 16 + 3 sums per tile, 7 floats per pixel"""
    scenes, (rows, cols) = c.batch or 1, c.size
    return (lib.dirt_background_scratch_bytes(scenes, rows, cols) // 4 - scenes * rows * cols * 7) // (19 * scenes)


def test_the_one_row_cases_stand_where_they_are_meant_to(lib):
    """One row of 300 pixels: two tiles of 256 x 1, and a gradient from both; the footprint case blends levels 0 and 1 of its cube
    on some pixels and clamps to level 0 on others; the batch has an operand of each kind per scene"""
    for name in ROWS_ONE:
        c = case(name)
        assert c.size[0] == 1 and tiles_of(lib, c) == 2
        go = c.go.reshape(-1, 300, 3)
        assert go[:, :256].any(axis=(1, 2)).all() and go[:, 256:].any(axis=(1, 2)).all()
        assert (c.ref['mass_d_matrix'] > 0).any() and (c.ref['mass_d_intensity'] > 0).all()
    c = case('row-footprint')
    assert len(c.levels) == 6 and c.kw['lod'] is None
    lower, two = c.ref['level'][c.keep], c.ref['two'][c.keep]
    assert (two & (lower == 0)).sum() >= 8 and (c.ref['lam'][c.keep] < 0).sum() >= 8      # levels 0 and 1, and the clamp at level 0
    c = case('row-batch')
    assert c.batch == 3 and c.M.shape == (3, 4, 4) and c.mask.shape == (3, 1, 300) and c.intensity.shape == (3, 3)


def test_the_many_tile_cases_stand_where_they_are_meant_to(lib):
    """260 tiles of one scene; 3 x 87 = 261 rows of three scenes into the one sum of a shared matrix and a shared intensity: the 256
    lanes of the reduction take a second turn.  Every tile holds a pixel that carries a gradient"""
    c = case('tiles-260')
    assert tiles_of(lib, c) == 260 and c.batch is None
    assert all(c.go[r:r + TILE, k:k + TILE].any() for r in (0, 16) for k in range(0, 2065, TILE))
    c = case('tiles-261')
    assert tiles_of(lib, c) == 87 and c.batch == 3 and c.M.shape == (4, 4) and c.intensity.shape == (3,) and c.mask.shape == (3, 33, 464)
    assert all(c.go[b, r:r + TILE, k:k + TILE].any() for b in range(3) for r in (0, 16, 32) for k in range(0, 464, TILE))
    for name in MANY_TILES:
        assert (case(name).ref['mass_d_matrix'][:, :] > 0).sum() >= 12 and (case(name).ref['mass_d_intensity'] > 0).all()


def test_the_large_cube_stands_where_it_is_meant_to():
    """A face of 64 x 64 texels does not fit the LDS patch: a tile whose pixels see one face sums into a patch that is a part of
    the face, and a tile that sees two faces scatters straight to memory.  lod = 0.6 touches levels 0 and 1 everywhere"""
    assert 64 * 64 > TEX_PATCH
    for name in LARGE:
        c = case(name)
        ref = c.ref
        fits = split = 0
        for r in range(0, 33, TILE):
            for k in range(0, 35, TILE):
                tile = np.s_[r:r + TILE, k:k + TILE]
                face = ref['face'][tile][ref['valid'][tile]]
                if len(np.unique(face)) > 1:
                    split += 1
                    continue
                used = 0
                for key in ('box0', 'box1'):
                    b = [x[tile][ref['valid'][tile]] for x in ref[key]]
                    if (b[0] >= 0).any():
                        used += (b[1].max() - b[0][b[0] >= 0].min() + 1) * (b[3].max() - b[2][b[2] >= 0].min() + 1)
                if used <= TEX_PATCH:
                    assert 0 < used < 64 * 64
                    fits += 1
        assert fits >= 1 and split >= 1, (name, fits, split)
    c = case('n64-lod')
    assert len(c.levels) == 7 and (c.ref['level'][c.keep] == 0).all() and c.ref['two'][c.keep].all()


def test_the_bad_operands_stand_where_they_are_meant_to():
    """A NaN entry of the matrix leaves no valid ray: zeros everywhere.  A NaN of the mask sits on a compared pixel that carries a
    gradient: that pixel, d matrix, d intensity and the texels it taps are NaN, its own d mask is not.  A mask of 2 weighs its pixel by -1.
    A NaN texel is tapped by compared pixels: they, their d mask, d matrix and its channel of d intensity are NaN, d environment is not"""
    c = case('nan-matrix')
    assert not c.ref['valid'].any() and c.share == 0.
    for k in ('out', 'd_matrix', 'd_intensity', 'd_mask'):
        assert not c.ref[k].any() and not c.ref['mass_' + k].any(), k
    assert not c.ref['d_levels'][0].any()
    c = case('nan-mask')
    ref = c.ref
    assert np.isnan(c.mask[NAN_PIXEL]) and np.isnan(c.mask).sum() == 1 and c.keep[NAN_PIXEL] and c.go[NAN_PIXEL].all()
    assert np.isnan(ref['out'][NAN_PIXEL]).all() and np.isnan(ref['out']).sum() == 3
    assert np.isnan(ref['d_matrix'])[:, :].sum() >= 12 and np.isnan(ref['d_intensity']).all() and np.isfinite(ref['d_mask']).all()
    assert 1 <= np.isnan(ref['d_levels'][0]).any(-1).sum() <= 4
    c = case('mask-two')
    assert c.mask[TWO_PIXEL] == 2. and c.keep[TWO_PIXEL] and c.go[TWO_PIXEL].all() and c.ref['out'][TWO_PIXEL].all()
    twin = make(432, BAD, rotation=1, mask=poisoned_mask(TWO_PIXEL, 0.))
    np.testing.assert_allclose(c.ref['out'][TWO_PIXEL], -twin.ref['out'][TWO_PIXEL], rtol=1e-12)
    assert all(np.isfinite(c.ref[k]).all() for k in ('out', 'd_matrix', 'd_intensity', 'd_mask'))
    c = case('nan-texel')
    ref = c.ref
    hit = np.isnan(ref['out']).any(-1)
    assert np.isnan(c.levels[0]).sum() == 1 and (hit & c.keep).sum() >= 1 and (np.isnan(ref['out'])[..., [0, 2]]).sum() == 0
    assert np.array_equal(np.isnan(ref['d_mask']), hit) and np.isnan(ref['d_intensity']).tolist() == [False, True, False]
    assert np.isnan(ref['d_matrix']).sum() >= 12 and np.isfinite(ref['d_levels'][0]).all() and ref['mass_d_levels'][0][NAN_TEXEL[:3]].all()


# ---- on the GPU

def _check(got, c, nans=False):
    worst = R.ratios(got, c.ref, c.operand)
    print({k: '%.2e' % v for k, v in worst.items()})
    for kind, x in worst.items():
        assert x == x and x <= KERNEL * F32[kind], (kind, x, KERNEL * F32[kind])
    dead = ~c.ref['valid']
    assert not got['out'][dead].any()      # no look-up: exactly 0
    if nans:
        same_nans(got, c)
    else:
        assert R.exact_where_massless(got, c.ref, c.operand)
        assert all(np.isfinite(v).all() for v in got.values())
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('name', ROWS_ONE + LARGE + ['mask-two'])
def test_kernels_against_the_restatement(gpu, name):
    c = case(name)
    got = run_kernel(c, gpu)
    assert got['out'].shape == (((c.batch,) if c.batch else ()) + tuple(c.size) + (3,))
    _check(got, c)


@pytest.mark.gpu
@pytest.mark.parametrize('name', MANY_TILES)
def test_more_rows_of_partial_sums_than_one_turn(gpu, name):
    """260 rows, and 261 rows of three scenes into one shared sum: within the bound, and every result but the environment's
    gradient (float atomics) the same bits on a second run"""
    c = case(name)
    a, b = run_kernel(c, gpu), run_kernel(c, gpu)
    _check(a, c)
    for k in ('out', 'd_matrix', 'd_intensity', 'd_mask'):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.gpu
def test_a_nan_in_the_matrix_leaves_exact_zeros(gpu):
    c = case('nan-matrix')
    got = run_kernel(c, gpu)
    for k, v in got.items():
        assert not v.any(), k      # (a NaN is non-zero)
    _check(got, c)


@pytest.mark.gpu
@pytest.mark.parametrize('name', WITH_NANS)
def test_a_nan_in_the_mask_or_the_environment(gpu, name):
    """The NaN of every result are the restatement's (of `out` and d mask off the kinks), everything else is within the bound"""
    _check(run_kernel(case(name), gpu), case(name), nans=True)


def _guarded(gpu, counts, pad, guard):
    return {k: torch.full((n + 2 * pad,), guard, dtype=torch.float32, device=gpu) for k, n in counts.items()}


@pytest.mark.gpu
def test_c_abi_on_a_batch_of_one_row_images(gpu, lib):
    """Three scenes of 1 x 300 with an operand of each kind per scene, every output and the scratch inside a larger buffer of a
    guard value: within the bound, nothing outside is written"""
    from dirt_amd import _lib
    c = case('row-batch')
    env, M, I, m, go = (_dev(gpu, x) for x in (R.pack(c.levels), c.M, c.intensity, c.mask, c.go))
    pad, guard, n = 37, -77.25, 3 * 300
    nbytes = lib.dirt_background_scratch_bytes(3, 1, 300)
    counts = dict(out=n * 3, d_environment=env.numel(), d_matrix=48, d_intensity=9, d_mask=n, scratch=nbytes // 4)
    bufs = _guarded(gpu, counts, pad, guard)
    at = lambda k: bufs[k].data_ptr() + 4 * pad   # noqa: E731
    tail = (3, 1, 300, 12, 1, 3, 3, 3, 1, _lib.BACKGROUND_FILTERS['bilinear'], 0., 0., 0, None)
    _lib.check(lib.dirt_background_forward(env.data_ptr(), M.data_ptr(), I.data_ptr(), m.data_ptr(), at('out'), *tail))
    _lib.check(lib.dirt_background_backward(env.data_ptr(), M.data_ptr(), I.data_ptr(), m.data_ptr(), go.data_ptr(), at('d_environment'), at('d_matrix'),
                                            at('d_intensity'), at('d_mask'), at('scratch'), nbytes, *tail))
    torch.cuda.synchronize()
    for k, count in counts.items():
        assert (bufs[k][:pad] == guard).all() and (bufs[k][pad + count:] == guard).all(), k
    shapes = dict(out=(3, 1, 300, 3), d_environment=(6, 12, 12, 3), d_matrix=(3, 4, 4), d_intensity=(3, 3), d_mask=(3, 1, 300))
    _check({k: bufs[k][pad:pad + counts[k]].cpu().numpy().reshape(shape) for k, shape in shapes.items()}, c)


@pytest.mark.gpu
def test_c_abi_on_an_empty_call(gpu, lib):
    """scenes = 3, rows = 0: both entry points succeed, the backward without scratch; the gradients of the environment, the
    matrices and the intensities are cleared to zero, and nothing is written past them or anywhere else"""
    from dirt_amd import _lib
    c = case('row-batch')
    env, M, I, m = (_dev(gpu, x) for x in (R.pack(c.levels), c.M, c.intensity, c.mask))
    pad, guard = 37, -77.25
    counts = dict(out=16, go=16, d_environment=env.numel(), d_matrix=48, d_intensity=9, d_mask=16)
    bufs = _guarded(gpu, counts, pad, guard)
    at = lambda k: bufs[k].data_ptr() + 4 * pad   # noqa: E731
    tail = (3, 0, 300, 12, 1, 3, 3, 3, 1, _lib.BACKGROUND_FILTERS['bilinear'], 0., 0., 0, None)
    assert lib.dirt_background_scratch_bytes(3, 0, 300) == 0
    _lib.check(lib.dirt_background_forward(env.data_ptr(), M.data_ptr(), I.data_ptr(), m.data_ptr(), at('out'), *tail))
    _lib.check(lib.dirt_background_backward(env.data_ptr(), M.data_ptr(), I.data_ptr(), m.data_ptr(), at('go'), at('d_environment'), at('d_matrix'),
                                            at('d_intensity'), at('d_mask'), None, 0, *tail))
    torch.cuda.synchronize()
    for k, count in counts.items():
        assert (bufs[k][:pad] == guard).all() and (bufs[k][pad + count:] == guard).all(), k
        inner = bufs[k][pad:pad + count]
        assert (inner == 0.).all() if k in ('d_environment', 'd_matrix', 'd_intensity') else (inner == guard).all(), k


if __name__ == '__main__':
    table, rows = measure()
    for name, share, worst in rows:
        print('%-14s share %.3f  %s' % (name, share, {k: '%.2e' % v for k, v in worst.items()}))
    print('F32 =', table)
