"""`texture.panorama_to_cube` / `texture.cube_to_panorama` (dirt_panorama.hip) where tests/test_panorama.py stops: more rows of
partial sums than one turn of d rotation's reduction takes; the instantiations S = 3, 4 with four channels, S = 4 into a
panorama and a cube whose faces are larger than the LDS patch, each on several tiles under a rotation; matrices that are no
rotations (sheared and mirrored, scaled by 2^+-20, 2^+-100 and 1e20, with a NaN or an Inf entry, all zeros); NaN and Inf texels;
the C ABI with every pointer at 4-byte alignment only; the wrapper's conversions and a captured call.

The method is tests/test_panorama.py's: tests/panorama_reference.py is the float64 reference, the float32 torch form's worst
|f32 - ref64| / mass per kind of result over THIS file's cases is the F32 table below (`python -m tests.test_panorama_edges`
prints it; `measure` makes it, with HEADROOM for the order of the torch form's own sums), the kernels get KERNEL times that,
an element of zero mass must be exact, the kinks are left out as there and no case leaves out more than a quarter.  The table is this file's own: a magnifying look-up (a cube of 48
texels under a panorama of 33 rows) multiplies the index error by the magnification, which the cases of the old table do not
reach, and growing the old table would loosen the old tests.  Each designed case has a test without a GPU that it stands where
it is meant to."""
import functools

import numpy as np
import pytest
import torch

from tests import panorama_reference as R
from tests.test_panorama import KERNEL, NAMES, TEX_PATCH, _dev, run_kernel

# python -m tests.test_panorama_edges
F32 = {'cube_out': 1.15e-4, 'cube_d_source': 3.38e-5, 'cube_d_rotation': 2.96e-8,
       'panorama_out': 4.23e-5, 'panorama_d_source': 3.52e-3, 'panorama_d_rotation': 8.64e-8}
HEADROOM = 1.1      # on the measured figures: the torch form adds its float32 sums in an order that depends on the machine's threads
TILE = 16

# sheared, scaled and mirrored: determinant -1.14
GENERAL = (np.array([[1.3, .2, 0.], [0., -.8, .1], [.3, 0., 1.1]]) @ R.rotation_matrix(R.ROTATIONS[1]).astype(np.float64)).astype(np.float32)
SCALES = {'2^20': 2.**20, '2^-20': 2.**-20, '2^100': 2.**100, '2^-100': 2.**-100, '1e20': 1e20}
POWERS = ('2^20', '2^-20', '2^100', '2^-100')


class Case(R.Case):
    """`R.Case` handed the matrix itself (float32 [3, 3]; it need be no rotation) and, in `poison`, values written over texels of
    the source by their flat index.  The kinks are judged by the float64 geometry alone, which no texel's value enters"""

    def __init__(self, to_cube, source_shape, sizes, samples, matrix, seed, poison=()):
        rng = np.random.default_rng(seed)
        self.to_cube, self.sizes, self.samples, self.turned = to_cube, sizes, samples, True
        self.source = rng.standard_normal(source_shape).astype(np.float32)
        for at, value in poison:
            self.source.reshape(-1)[at] = value
        self.rotation = np.ascontiguousarray(matrix, np.float32)
        with np.errstate(invalid='ignore'):
            plain = self.run(None)
        self.excluded = plain['kink']
        self.share = float(self.excluded.mean())
        self.valid = plain['valid']
        go = rng.standard_normal(plain['out'].shape).astype(np.float32)
        go[self.excluded] = 0.
        self.go = go

    @functools.cached_property
    def ref(self):
        with np.errstate(invalid='ignore'):
            return self.run(self.go)


def rot(k):
    return R.rotation_matrix(R.ROTATIONS[k])


def scaled(k, scale):
    return (rot(k).astype(np.float64) * scale).astype(np.float32)


SCALE_CUBE = (True, (7, 13, 3), 5, 3)            # the shapes of 'n5-s3-r1' and 'q17x33'
SCALE_PANO = (False, (6, 4, 4, 4), (17, 33), 2)
# a NaN and an Inf texel away from the clamped rows (a clamped row gives its second row a weight of exactly 0)
NAN_PANO = [((4 * 20 + 7) * 3 + 1, np.nan), ((5 * 20 + 15) * 3 + 0, np.inf)]
NAN_CUBE = [(((2 * 6 + 2) * 6 + 3) * 3 + 1, np.nan), (((5 * 6 + 3) * 6 + 2) * 3 + 2, np.inf)]

_CASES = {
    'rows-294': lambda: Case(True, (32, 64, 3), 97, 1, rot(1), 100),                 # 6 x 49 tiles
    'rows-260': lambda: Case(False, (6, 8, 8, 1), (17, 2065), 1, rot(1), 101),        # 2 x 130 tiles
    's3-c4': lambda: Case(True, (9, 20, 4), 17, 3, rot(1), 110),
    's4-c3': lambda: Case(True, (9, 20, 3), 17, 4, rot(2), 111),
    'q-s4-c3': lambda: Case(False, (6, 6, 6, 3), (17, 33), 4, rot(2), 112),
    'q-n48': lambda: Case(False, (6, 48, 48, 4), (33, 65), 2, rot(0), 113),           # a face of 2304 texels: per-tile patches
    'general': lambda: Case(True, (9, 20, 3), 17, 2, GENERAL, 120),
    'q-general': lambda: Case(False, (6, 17, 17, 3), (17, 33), 2, GENERAL, 121),
    'scale': lambda: Case(*SCALE_CUBE, rot(1), 130),
    'q-scale': lambda: Case(*SCALE_PANO, rot(0), 131),
    **{'scale:' + s: (lambda s=s: Case(*SCALE_CUBE, scaled(1, SCALES[s]), 130)) for s in SCALES},
    **{'q-scale:' + s: (lambda s=s: Case(*SCALE_PANO, scaled(0, SCALES[s]), 131)) for s in SCALES},
    'nan-texels': lambda: Case(True, (9, 20, 3), 17, 2, rot(0), 140, NAN_PANO),
    'q-nan-texels': lambda: Case(False, (6, 6, 6, 3), (17, 33), 2, rot(0), 141, NAN_CUBE),
}
ROWS = ['rows-294', 'rows-260']
INSTANCES = ['s3-c4', 's4-c3', 'q-s4-c3', 'q-n48']
GENERALS = ['general', 'q-general']
MAGNITUDES = ['scale', 'q-scale'] + ['scale:' + s for s in SCALES] + ['q-scale:' + s for s in SCALES]
POISONED = ['nan-texels', 'q-nan-texels']
RESTATED = ROWS + INSTANCES + GENERALS + MAGNITUDES      # held to the table in every kind of result


@functools.lru_cache(maxsize=None)
def case(name):
    return _CASES[name]() if name in _CASES else R.case(name)


def bound(c, kind, factor=1):
    return factor * F32[('cube_' if c.to_cube else 'panorama_') + kind]


def finite_ratios(got, c):
    """`R.ratios` for a case with texels that are not finite: `out` over the compared elements whose reference is finite,
    d source (which no texel's value enters) in full"""
    ref = c.ref
    keep = np.broadcast_to(~c.excluded[..., None], ref['out'].shape) & np.isfinite(ref['out'])
    return {'out': R.worst_ratio(np.where(keep, got['out'], 0.), np.where(keep, ref['out'], 0.), np.where(keep, ref['mass_out'], 0.), keep),
            'd_source': R.worst_ratio(got['d_source'], ref['d_source'], ref['mass_d_source'])}


def measure():
    """-> the table: the float32 torch form's worst ratio per kind of result over this file's cases, and per case its figures"""
    table, rows = {}, []
    for name in RESTATED + POISONED:
        c = case(name)
        worst = finite_ratios(R.torch_form(c), c) if name in POISONED else R.ratios(R.torch_form(c), c)
        rows.append((name, c.share, worst))
        for k, v in worst.items():
            key = ('cube_' if c.to_cube else 'panorama_') + k
            table[key] = max(table.get(key, 0.), v)
    return {k: float('%.2e' % (v * HEADROOM)) for k, v in sorted(table.items())}, rows


# ---- without a GPU

@pytest.mark.parametrize('name', RESTATED)
def test_the_float32_torch_form_against_the_restatement(name):
    """Per element, relative to the element's mass: within this file's F32 table, whose figures are this test's own worst ones"""
    c = case(name)
    got = R.torch_form(c)
    worst = R.ratios(got, c)
    print(name, {k: '%.2e' % v for k, v in worst.items()})
    for kind, x in worst.items():
        assert x <= bound(c, kind), (kind, x)
    assert R.exact_where_massless(got, c)


def test_no_case_leaves_out_more_than_a_quarter():
    """... and the designed ones stay near the shares measured beforehand (at most 0.07)"""
    for name in RESTATED + POISONED:
        assert case(name).share <= 0.25, (name, case(name).share)
    for name in ROWS + INSTANCES + GENERALS:
        assert case(name).share <= 0.08, (name, case(name).share)


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import _lib
    return _lib.load()


def tiles_of(lib, c):
    """the rows of partial sums of the case's backward, from the scratch the library asks for"""
    if c.to_cube:
        return lib.dirt_panorama_scratch_bytes(c.source.shape[0], c.source.shape[1], c.sizes, c.source.shape[-1], c.samples, 1) // (4 * 9)
    (h, w), ct, s = c.sizes, c.source.shape[-1], c.samples
    return (lib.dirt_panorama_scratch_bytes(h, w, c.source.shape[1], ct, s, 0) // 4 - h * s * w * s * (3 + ct)) // 9


def test_the_row_cases_stand_where_they_are_meant_to(lib):
    """More than 256 rows of nine partial sums each: the 256 lanes of the reduction take a second turn; every row's tile holds a
    texel that carries a gradient"""
    assert tiles_of(lib, case('rows-294')) == 6 * 49 == 294 and tiles_of(lib, case('rows-260')) == 2 * 130 == 260
    for name in ROWS:
        c = case(name)
        assert c.valid.all() and (c.ref['mass_d_rotation'] > 0).all()
    go = case('rows-294').go
    assert all(go[f, r:r + TILE, k:k + TILE].any() for f in range(6) for r in range(0, 97, TILE) for k in range(0, 97, TILE))
    go = case('rows-260').go
    assert all(go[r:r + TILE, k:k + TILE].any() for r in (0, 16) for k in range(0, 2065, TILE))


def cube_taps(q, n):
    """face, r0, r1, c0, c1 of the bilinear cube look-ups of directions q [M, 3] (float64)"""
    ad = np.abs(q)
    major = np.where((ad[:, 0] >= ad[:, 1]) & (ad[:, 0] >= ad[:, 2]), 0, np.where(ad[:, 1] >= ad[:, 2], 1, 2))
    face = 2 * major + (q[np.arange(len(q)), major] <= 0)
    a = (q * R.FACE_M[face]).sum(-1)
    lo = [np.floor(np.clip((((q * axis[face]).sum(-1) / a + 1) * 0.5) * n - 0.5, 0, n - 1)).astype(int) for axis in (R.FACE_T, R.FACE_S)]
    return (face, lo[0], np.minimum(lo[0] + 1, n - 1), lo[1], np.minimum(lo[1] + 1, n - 1))


def test_the_instances_stand_where_they_are_meant_to(lib):
    """Several tiles each (the last ones partial); S and the channel count as named; in 'q-n48' a face holds more texels than
    the LDS patch, a tile of the scatter (16 x 16 samples) whose look-ups lie on one face has a box that fits the patch and is
    not the face, and another tile's look-ups lie on two faces: both ways of the scatter, on patches of a face"""
    for name, tiles, s, ct in (('s3-c4', 24, 3, 4), ('s4-c3', 24, 4, 3), ('q-s4-c3', 6, 4, 3), ('q-n48', 15, 2, 4)):
        c = case(name)
        assert tiles_of(lib, c) == tiles and c.samples == s and c.source.shape[-1] == ct and c.valid.all(), name
        assert (c.ref['mass_d_rotation'] > 0).all()
    c = case('q-n48')
    n, s = 48, 2
    assert n * n > TEX_PATCH
    q = R.panorama_sample_directions(33, 65, s) @ c.rotation.astype(np.float64)
    fits = split = 0
    for r in range(0, 33 * s, TILE):
        for k in range(0, 65 * s, TILE):
            face, r0, r1, c0, c1 = cube_taps(q[r:r + TILE, k:k + TILE].reshape(-1, 3), n)
            box = (r1.max() - r0.min() + 1) * (c1.max() - c0.min() + 1)
            if len(np.unique(face)) > 1:
                split += 1
            elif box <= TEX_PATCH:
                assert box < n * n
                fits += 1
    assert fits >= 8 and split >= 8, (fits, split)


def test_the_general_matrix_is_no_rotation():
    """Sheared (its rows are not orthogonal), scaled (nor of length 1) and mirrored (determinant -1.14); all three results
    have a mass everywhere they could"""
    G = GENERAL.astype(np.float64)
    assert abs(np.linalg.det(G) + 1.138) < 1e-3      # 1.3 (-0.8 x 1.1) - 0.2 (-0.1 x 0.3) = -1.138
    gram = G @ G.T
    assert np.abs(gram - np.diag(np.diag(gram))).max() > 0.1 and np.abs(np.diag(gram) - 1.).min() > 0.2
    for name in GENERALS:
        c = case(name)
        assert c.valid.all() and (c.ref['mass_d_rotation'] > 0).all() and np.array_equal(c.rotation, GENERAL)


def test_the_magnitude_cases_stand_where_they_are_meant_to():
    """The scaled matrices are the base's times the scale (a power of two: exactly), their cases share the base's source, the
    elements left out and the incoming gradient, and without the scaling x x + z z would overflow (2^100, 1e20) or underflow
    (2^-100) in float32"""
    for stem, k in (('scale', 1), ('q-scale', 0)):
        base = case(stem)
        assert base.valid.all()
        for s, scale in SCALES.items():
            c = case('%s:%s' % (stem, s))
            assert np.array_equal(c.source, base.source) and np.array_equal(c.excluded, base.excluded) and np.array_equal(c.go, base.go), (stem, s)
            assert np.isfinite(c.rotation).all() and c.valid.all()
            if s in POWERS:
                assert np.array_equal(c.rotation.astype(np.float64), base.rotation.astype(np.float64) * scale)
    with np.errstate(over='ignore', under='ignore'):
        assert np.isinf(np.float32(2.**100) * np.float32(2.**100)) and np.isinf(np.float32(1e20) * np.float32(1e20))
        assert np.float32(2.**-100) * np.float32(2.**-100) == 0.


LOOKS = [(1., 1., 0.), (0.3, -0.2, 0.9), (-2., 0.5, -0.25), (0., -1., 3.), (1e-3, 5., -2e-3)]


def test_the_length_of_a_direction_does_not_matter():
    """`directions_to_panorama_indices` at 2^+-30, 2^+-100 times a direction: the indices of the direction itself to the bit, and
    the gradient times the inverse power; at 1e20 and 1e-25 (whose products round) to float32 rounding.  (1, 1, 0) on 8 x 16 is
    index (1.5, 11.5) at every length: x x + z z overflowed to the equator (3.5, 11.5) at 1e20 and underflowed to the pole
    (0, 7.5) at 1e-25"""
    from dirt_amd import texture
    d = torch.tensor(LOOKS)
    weights = torch.tensor([[0.7, -1.3]])

    def look(scale):
        x = (d * scale).requires_grad_(True)
        idx, valid = texture.directions_to_panorama_indices(x, 8, 16)
        (idx * weights).sum().backward()
        assert valid.all()
        return idx.detach(), x.grad

    idx, grad = look(1.)
    assert idx[0].tolist() == [1.5, 11.5]
    for p in (30, -30, 100, -100):
        i, g = look(2.**p)
        assert torch.equal(i, idx) and torch.equal(g, grad * 2.**-p), p
    for scale in (1e20, 1e-25):
        i, g = look(scale)
        assert torch.allclose(i, idx, rtol=0, atol=1e-5) and torch.allclose(g * scale, grad, rtol=1e-5, atol=1e-6), scale
        assert (i[0] - idx[0]).abs().max() <= 2e-6


def test_a_subnormal_direction_is_looked_up_like_its_multiple():
    """A largest component that is subnormal (2^-140, and 5 x 2^-149: the last bits of float32) is scaled in two steps, 2^148
    being no float32: the indices of the same direction times 2^140 or 2^149, to the bit"""
    from dirt_amd import texture
    small = torch.tensor([[1., 1., 0.], [3., -2., 5.], [0., 1., 0.], [-1., 0., 4.]])
    for p in (140, 147):
        tiny = small * 2.**-p
        assert (tiny.abs().amax(-1) < float(np.finfo(np.float32).tiny)).all() and torch.equal(tiny.double() * 2.**p, small.double())
        idx, valid = texture.directions_to_panorama_indices(tiny, 8, 16)
        want, _ = texture.directions_to_panorama_indices(small, 8, 16)
        assert valid.all() and torch.equal(idx, want), p
    last = torch.tensor([[3., -2., 5.]]) * 2.**-149
    idx, valid = texture.directions_to_panorama_indices(last, 8, 16)
    assert valid.all() and torch.equal(idx, texture.directions_to_panorama_indices(torch.tensor([[3., -2., 5.]]), 8, 16)[0])


def test_a_power_of_two_times_the_matrix_gives_the_bits_of_the_matrix():
    """The dense forms' three results under 2^+-100 R: the unscaled call's to the bit, d rotation times 2^-+100"""
    for stem in ('scale', 'q-scale'):
        base = R.torch_form(case(stem))
        for s, p in (('2^100', 100), ('2^-100', -100)):
            got = R.torch_form(case('%s:%s' % (stem, s)))
            assert np.array_equal(got['out'], base['out']) and np.array_equal(got['d_source'], base['d_source']), (stem, s)
            assert np.array_equal(got['d_rotation'], base['d_rotation'] * np.float32(2.**-p)), (stem, s)


BAD_MATRICES = {'nan': (4, np.nan), 'inf': (2, np.inf), 'zeros': None}


def bad_matrix(kind):
    if kind == 'zeros':
        return np.zeros((3, 3), np.float32)
    M = rot(1).copy()
    M.reshape(-1)[BAD_MATRICES[kind][0]] = BAD_MATRICES[kind][1]
    return M


@pytest.mark.parametrize('kind', list(BAD_MATRICES))
def test_a_matrix_that_is_not_finite_leaves_no_valid_sample(kind):
    """One NaN entry, one Inf entry, or all zeros: every sample's direction has a component that is not finite, or is all zero.
    The restatement and the float32 torch form give zeros in all three results, both ways"""
    for stem in ('scale', 'q-scale'):
        base = case(stem)
        c = Case(base.to_cube, base.source.shape, base.sizes, base.samples, bad_matrix(kind), 150)
        assert not c.valid.any() and c.share == 0.
        got = R.torch_form(c)
        for k in R.KINDS:
            assert not c.ref[k].any() and not c.ref['mass_' + k].any() and not got[k].any(), (stem, k)      # (a NaN is non-zero)


@pytest.mark.parametrize('name', POISONED)
def test_texels_that_are_not_finite_stand_where_they_are_meant_to(name):
    """One NaN and one Inf texel, both under compared elements that carry a gradient: the restatement's `out` holds NaN, +Inf and
    finite elements, its d rotation is NaN throughout and its d source finite; the float32 torch form agrees: the same elements
    NaN and +Inf off the kinks, the others and d source within the table"""
    c = case(name)
    ref = c.ref
    keep = np.broadcast_to(~c.excluded[..., None], ref['out'].shape)
    assert (np.isnan(ref['out']) & keep).sum() >= 1 and (np.isposinf(ref['out']) & keep).sum() >= 1 and not np.isneginf(ref['out']).any()
    assert np.isfinite(ref['out']).mean() > 0.9
    assert np.isnan(ref['d_rotation']).all() and np.isfinite(ref['d_source']).all()
    assert (~np.isfinite(c.source)).sum() == 2 and (ref['mass_d_source'][~np.isfinite(c.source)] > 0).all()
    got = R.torch_form(c)
    same_pattern(got, c)
    for kind, x in finite_ratios(got, c).items():
        assert x <= bound(c, kind), (kind, x)


def same_pattern(got, c):
    ref = c.ref
    keep = np.broadcast_to(~c.excluded[..., None], ref['out'].shape)
    assert np.array_equal(np.isnan(got['out'])[keep], np.isnan(ref['out'])[keep])
    assert np.array_equal(np.isposinf(got['out'])[keep], np.isposinf(ref['out'])[keep]) and not np.isneginf(got['out'])[keep].any()
    assert np.isnan(got['d_rotation']).all() and np.isfinite(got['d_source']).all()


# ---- on the GPU

def _check(got, c):
    worst = R.ratios(got, c)
    print({k: '%.2e' % v for k, v in worst.items()})
    for kind, x in worst.items():
        assert x == x and x <= bound(c, kind, KERNEL), (kind, x, bound(c, kind, KERNEL))
    assert R.exact_where_massless(got, c)
    assert all(np.isfinite(v).all() for v in got.values())
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('name', ROWS)
def test_more_rows_of_partial_sums_than_one_turn(gpu, name):
    """294 and 260 rows into d rotation's nine sums: within the bound, and the same bits in `out` and d rotation on a second run"""
    c = case(name)
    a, b = run_kernel(c, gpu), run_kernel(c, gpu)
    _check(a, c)
    assert np.array_equal(a['out'], b['out']) and np.array_equal(a['d_rotation'], b['d_rotation'])


@pytest.mark.gpu
@pytest.mark.parametrize('name', INSTANCES + GENERALS)
def test_kernels_against_the_restatement(gpu, name):
    c = case(name)
    got = run_kernel(c, gpu)
    assert got['out'].shape == c.ref['out'].shape and got['d_source'].shape == c.source.shape and got['d_rotation'].shape == (3, 3)
    _check(got, c)


@pytest.mark.gpu
@pytest.mark.parametrize('stem', ['scale', 'q-scale'])
def test_the_length_of_the_matrix_does_not_matter(gpu, stem):
    """2^+-20, 2^+-100 times the rotation: `out` to the bit and the same set of non-zero elements of d source as the unscaled
    call's; these and 1e20 times it: all three results within the bound of the restatement of the scaled matrix"""
    base = case(stem)
    plain = run_kernel(base, gpu)
    _check(plain, base)
    for s in SCALES:
        c = case('%s:%s' % (stem, s))
        got = run_kernel(c, gpu)
        print(stem, s, end=' ')
        _check(got, c)
        if s in POWERS:
            assert np.array_equal(got['out'], plain['out']), s
            assert np.array_equal(got['d_source'] != 0, plain['d_source'] != 0), s


@pytest.mark.gpu
def test_a_subnormal_direction_on_the_gpu(gpu):
    """2^-140 times a signed permutation, a cube of 8 texels, one sample each: every component of every direction is a multiple of
    2^-143, held exactly; `out` is the unscaled call's to the bit both ways (the cube look-up divides by the major axis)"""
    from dirt_amd import texture
    P = np.array([[0., 0., 1.], [-1., 0., 0.], [0., 1., 0.]], np.float32)
    rng = np.random.default_rng(160)
    pan, cube = (_dev(gpu, rng.standard_normal(shape).astype(np.float32)) for shape in ((9, 20, 3), (6, 8, 8, 3)))
    tiny = _dev(gpu, P * np.float32(2.**-140))
    assert 0. < float(tiny.abs().max()) < float(np.finfo(np.float32).tiny)
    a, b = (texture.panorama_to_cube(pan, 8, samples=1, rotation=r) for r in (_dev(gpu, P), tiny))
    assert torch.equal(a, b) and a.abs().sum() > 0
    cube_dirs = R.cube_sample_directions(8, 1).reshape(-1, 3) @ P.astype(np.float64).T
    want = R.look_panorama(pan.cpu().numpy().astype(np.float64), cube_dirs)
    keep = ~want['kink']
    assert R.worst_ratio(b.cpu().numpy().reshape(-1, 3)[keep], want['value'][keep], want['mass'][keep]) <= KERNEL * F32['cube_out']


@pytest.mark.gpu
@pytest.mark.parametrize('kind', list(BAD_MATRICES))
def test_a_matrix_that_is_not_finite_gives_exact_zeros(gpu, kind):
    """No valid look-up in any tile (no patch, no scatter): `out` and both gradients are exact zeros, both ways"""
    for stem in ('scale', 'q-scale'):
        base = case(stem)
        got = run_kernel(base, gpu, rotation=_dev(gpu, bad_matrix(kind)).requires_grad_(True))
        for k in R.KINDS:
            assert got[k].shape == base.ref[k].shape and not got[k].any(), (stem, k)      # (a NaN is non-zero)


@pytest.mark.gpu
@pytest.mark.parametrize('name', POISONED)
def test_texels_that_are_not_finite(gpu, name):
    """Off the excluded elements the NaN and Inf elements of `out` are the restatement's, the others within the bound; d rotation
    is NaN throughout; d source, which no texel's value enters, is finite and within its bound"""
    c = case(name)
    got = run_kernel(c, gpu)
    same_pattern(got, c)
    worst = finite_ratios(got, c)
    print(worst)
    for kind, x in worst.items():
        assert x == x and x <= bound(c, kind, KERNEL), (kind, x)
    assert not got['d_source'][c.ref['mass_d_source'] == 0].any()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['n8-s2-r0', 'q17x33'])
def test_c_abi_with_every_pointer_at_four_byte_alignment(gpu, lib, name):
    """Four channels (the kernels move a texel as one 16-byte piece) with the source, the rotation, grad_out, every output and the
    scratch one float past a 16-byte boundary, guard values around the outputs: within the bound, nothing outside is written"""
    from dirt_amd import texture
    c = case(name)
    assert c.source.shape[-1] == 4
    pad, guard = 37, -77.25      # 148 bytes: 4 past a multiple of 16
    stem = NAMES[0] if c.to_cube else NAMES[1]
    rows, cols = c.source.shape[:2] if c.to_cube else c.sizes
    size, ct = (c.sizes if c.to_cube else c.source.shape[1]), 4
    tail = (rows, cols, size, ct, c.samples, None)
    nbytes = lib.dirt_panorama_scratch_bytes(rows, cols, size, ct, c.samples, int(c.to_cube))
    counts = dict(source=c.source.size, rotation=9, go=c.go.size, out=c.go.size, d_source=c.source.size, d_rotation=9, scratch=nbytes // 4)
    bufs = {k: torch.full((n + 2 * pad,), guard, dtype=torch.float32, device=gpu) for k, n in counts.items()}
    for k, x in (('source', c.source), ('rotation', c.rotation), ('go', c.go)):
        bufs[k][pad:pad + counts[k]] = _dev(gpu, x).reshape(-1)
    at = lambda k: bufs[k].data_ptr() + 4 * pad   # noqa: E731
    assert all(at(k) % 16 == 4 for k in bufs)
    texture._check(getattr(lib, stem + '_forward')(at('source'), at('rotation'), at('out'), *tail))
    texture._check(getattr(lib, stem + '_backward')(at('source'), at('rotation'), at('go'), at('d_source'), at('d_rotation'), at('scratch'), nbytes, *tail))
    torch.cuda.synchronize()
    for k, n in counts.items():
        assert (bufs[k][:pad] == guard).all() and (bufs[k][pad + n:] == guard).all(), k
    shapes = dict(out=c.go.shape, d_source=c.source.shape, d_rotation=(3, 3))
    got = {k: bufs[k][pad:pad + counts[k]].cpu().numpy().reshape(shape) for k, shape in shapes.items()}
    worst = R.ratios(got, c)
    from tests.test_panorama import F32 as OLD      # the cases are the old file's, and so is their table
    for kind, x in worst.items():
        assert x == x and x <= KERNEL * OLD[('cube_' if c.to_cube else 'panorama_') + kind], (kind, x)
    assert R.exact_where_massless(got, c)


# ---- the wrappers

def _call(c, src, rotation):
    from dirt_amd import texture
    if c.to_cube:
        return texture.panorama_to_cube(src, c.sizes, samples=c.samples, rotation=rotation)
    return texture.cube_to_panorama(src, c.sizes[0], c.sizes[1], samples=c.samples, rotation=rotation)


@pytest.mark.gpu
@pytest.mark.parametrize('stem', ['scale', 'q-scale'])
def test_float64_and_float16_operands(gpu, stem):
    """A float64 source with a float64 rotation: `out` is float32 with the float32 call's bits, the gradients come back in their
    operand's dtype and shape, d rotation the float32 bits, d source within the bound.  A float16 source (the case's rounded to
    float16): the float32 call on the same values likewise, d source to the rounding of a float16 on top of the bound (half an
    ulp, 2^-11 of the value, or half the smallest subnormal, 2^-25)"""
    base = case(stem)
    rounded = base.source.astype(np.float16)
    c16 = Case(base.to_cube, base.source.shape, base.sizes, base.samples, base.rotation, 130 if base.to_cube else 131)
    c16.source = rounded.astype(np.float32)
    assert np.array_equal(c16.go, base.go)
    for c, dtype, slack in ((base, torch.float64, 0.), (c16, torch.float16, 1.)):
        dense = run_kernel(c, gpu)
        _check(dense, c)
        src = _dev(gpu, c.source).to(dtype).requires_grad_(True)
        rotation = _dev(gpu, c.rotation).double().requires_grad_(True)
        out = _call(c, src, rotation)
        assert out.dtype == torch.float32 and np.array_equal(out.detach().cpu().numpy(), dense['out'])
        d_src, d_rot = torch.autograd.grad(out, (src, rotation), _dev(gpu, c.go))
        assert d_src.dtype == dtype and d_src.shape == src.shape and d_rot.dtype == torch.float64 and d_rot.shape == (3, 3)
        assert np.array_equal(d_rot.cpu().numpy(), dense['d_rotation'].astype(np.float64))
        ref = c.ref
        excess = np.abs(d_src.cpu().numpy().astype(np.float64) - ref['d_source']) \
            - (bound(c, 'd_source', KERNEL) * ref['mass_d_source'] + slack * (2.**-11 * np.abs(ref['d_source']) + 2.**-25))
        assert (excess <= 0.).all(), (dtype, excess.max())


@pytest.mark.gpu
@pytest.mark.parametrize('stem', ['scale', 'q-scale'])
def test_a_captured_call_replays_on_a_new_source_and_a_new_rotation(gpu, stem):
    """The call and its backward captured with torch.cuda.graph and replayed twice, the source and the rotation rewritten in place
    before each replay: `out` and d rotation are the eager call's bits on the same operands, d source (float atomics; cleared by
    the library on every replay) within the bound"""
    first = case(stem)
    src, rotation, go = (_dev(gpu, x) for x in (first.source, first.rotation, first.go))

    def step():
        leaves = [x.detach().requires_grad_(True) for x in (src, rotation)]
        out = _call(first, *leaves)
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
    for k in (2, 0):
        other = Case(first.to_cube, first.source.shape, first.sizes, first.samples, rot(k), 170 + k)
        other.go = np.where(other.excluded[..., None], np.float32(0.), first.go)      # the captured gradient, zero on this one's kinks too
        with torch.no_grad():
            src.copy_(_dev(gpu, other.source))
            rotation.copy_(_dev(gpu, other.rotation))
            go.copy_(_dev(gpu, other.go))
        graph.replay()
        torch.cuda.synchronize()
        got = dict(zip(R.KINDS, (x.cpu().numpy() for x in captured)))
        eager = run_kernel(other, gpu, go=_dev(gpu, other.go))
        assert np.array_equal(got['out'], eager['out']) and np.array_equal(got['d_rotation'], eager['d_rotation']), k
        _check(got, other)


if __name__ == '__main__':
    table, rows = measure()
    for name, share, worst in rows:
        print('%-16s share %.3f  %s' % (name, share, {k: '%.2e' % v for k, v in worst.items()}))
    print('F32 =', table)
