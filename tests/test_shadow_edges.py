"""`shading.shadow_visibility` (dirt_shadow.hip) where tests/test_shadow.py stops: more tiles than one turn of the matrices'
reduction takes, tile grids with unequal sides and partial tiles, images of one column, two rows and one row; LDS patches
anchored off texel (0, 0), a light whose box fits the patch next to one whose box does not, direct atomics into per-scene maps;
non-finite and out-of-range points and non-finite texels on the GPU; a softness far below the depth noise and at the ends of
float32; the wrapper's conversions, copies and a second backward.  Cases, tolerances and helpers are tests/test_shadow.py's:
what is compared with the float64 restatement is held to KERNEL x F32 per element against its L1 mass (`_check`), and every
case held to it is part of `tolerance_cases`, which the F32 table is measured on.  Each designed case has a test without a GPU
that it stands where it is meant to, from the float64 values of its inputs alone."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import shadow_reference as R
from tests.test_shadow import Case, grid_case, random_case, _run, _check, _dev, KERNEL, F32, TILE, SHADOW_BLOCK, TEX_PATCH
from tests.test_shadow import case as base_case

FLT_MIN = float(np.finfo(np.float32).tiny)


def scale(s):
    """x and y scaled about the map's centre (row vectors: clip = [q, 1] @ M)"""
    return np.diag([s, s, 1., 1.]).astype(np.float32)


def redrawn(base, maps, mats, seed, kw=None):
    """`base` with other maps and matrices: the pixels these put within OFF_KINKS of a kink are drawn again"""
    rng = np.random.default_rng(seed)
    kw = kw or base.kw
    g = base.g.copy()
    for _ in range(40):
        bad = R.compose(g, maps, mats, base.layout, masses=False, **kw)['kink'] < R.OFF_KINKS
        if not bad.any():
            return Case(base.shape, g, maps, mats, base.layout, kw, seed + 1)
        assert bad.mean() < 0.5
        g[bad] = R.random_pixels(rng, int(bad.sum()), g.shape[1], base.layout)
    raise AssertionError('could not draw pixels off the kinks')


# ---- the cases

OFFSET_MAP = (64, 56)
OFFSET_ROWS, OFFSET_COLS = 17.35 + np.arange(TILE) * 1.9, 23.45 + np.arange(TILE) * 1.9                 # one tile from texel (17, 23); fractions 0.05 .. 0.95
TILES_ROWS, TILES_COLS = 17.3 + np.arange(2 * TILE) * 0.93, 23.4 + np.arange(2 * TILE) * 0.91         # 32 x 32 pixels over the same texels
MIXED_STEPS = 0.7 + np.arange(TILE) * 2.59                                                              # 41 x 41 texels of a 48 x 48 map under the identity
BATCH_STEPS = 0.45 + np.arange(TILE) * 2.6       # fractions no nearer than 0.04 to a texel centre under either matrix: fr = row - floor(row) keeps its bits
BAD_SHAPE = (17, 19)


def hard_case():
    """The geometry of 'image' (its maps, matrices, layout, kernel) with softness 1e-6: pixels drawn until every window of every
    light is flat by a margin -- flat already at a softness of 1e-3, so that no float32 rounding of Z - d (1e-7) brings a
    comparison back between 0 and 1"""
    base = base_case('image')
    rng = np.random.default_rng(700)
    n = int(np.prod(base.shape))
    kw, wide = dict(base.kw, softness=1.e-6), dict(base.kw, softness=1.e-3)
    chosen = []
    for _ in range(60):
        pool = R.random_pixels(rng, 4 * n, base.g.shape[1], base.layout)
        pool[:, base.layout[0] + 2] *= 1.5
        a, b = (R.compose(pool, base.maps, base.mats, base.layout, masses=False, **k) for k in (wide, kw))
        keep = a['flat'] & b['flat'] & (a['kink'] >= R.OFF_KINKS) & (b['kink'] >= R.OFF_KINKS)
        chosen.append(pool[keep])
        if sum(len(x) for x in chosen) >= n:
            return Case(base.shape, np.concatenate(chosen)[:n], base.maps, base.mats, base.layout, kw, 701)
    raise AssertionError('could not draw flat pixels')


@functools.lru_cache(maxsize=None)
def case(name):
    if name == 'many-tiles-image':
        return random_case(400, (2, 257 * TILE), 8, (1, 4, 0), 2, 12, 10, 3, normal_offset=0.04)
    if name == 'many-tiles-image-2':       # a second scene over the same maps and matrices
        c = case('many-tiles-image')
        g, _ = R.draw_off_kinks(np.random.default_rng(402), c.g.shape[0], 8, c.layout, c.maps, c.mats, c.kw)
        return Case(c.shape, g, c.maps, c.mats, c.layout, c.kw, 403)
    if name == 'many-tiles-flat':
        return random_case(410, (256 * SHADOW_BLOCK + 3,), 8, (1, 4, 0), 1, 16, 16, 1)
    if name == 'grid-3x4':
        return random_case(420, (35, 50), 9, (6, 3, 2), 3, 11, 13, 5, normal_offset=0.03)
    if name == 'column':
        return random_case(430, (37, 1), 8, (1, 4, 0), 2, 9, 7, 3, normal_offset=0.05)
    if name == 'two-rows':
        return random_case(431, (2, 19), 8, (1, 4, 0), 2, 9, 7, 3)
    if name == 'one-row':
        return random_case(432, (1, SHADOW_BLOCK + 3), 8, (1, 4, 0), 2, 9, 7, 3, normal_offset=0.05)
    if name == 'one-row-2':
        c = case('one-row')
        g, _ = R.draw_off_kinks(np.random.default_rng(433), c.g.shape[0], 8, c.layout, c.maps, c.mats, c.kw)
        return Case(c.shape, g, c.maps, c.mats, c.layout, c.kw, 434)
    if name.startswith('patch-offset-'):
        if name == 'patch-offset-tiles':
            return grid_case(510, (2 * TILE, 2 * TILE), *OFFSET_MAP, TILES_ROWS[:, None], TILES_COLS[None, :], 3)
        kernel = int(name[-1])
        return grid_case(500 + kernel, (TILE, TILE), *OFFSET_MAP, OFFSET_ROWS[:, None], OFFSET_COLS[None, :], kernel)
    if name == 'patch-mixed':              # fits, does not, fits again
        return grid_case(520, (TILE, TILE), 48, 48, MIXED_STEPS[:, None], MIXED_STEPS[None, :], 1, mats=[scale(0.55), scale(1.), scale(0.8)])
    if name == 'patch-mixed-reversed':
        return grid_case(521, (TILE, TILE), 48, 48, MIXED_STEPS[:, None], MIXED_STEPS[None, :], 1, mats=[scale(1.), scale(0.55)])
    if name.startswith('direct-batch-'):   # scene 0 from texel 0.45, scene 1 from texel 6.55: 41 or 42 texels a side under either light
        b = int(name[-1])
        steps = BATCH_STEPS + 6.1 * b
        return grid_case(530 + b, (TILE, TILE), 48, 48, steps[:, None], steps[None, :], 1, mats=[scale(1.), scale(1.03)])
    if name.startswith('flat-'):           # the first n pixels of 'flat'
        c, n = base_case('flat'), int(name.split('-')[1])
        return Case((n,), c.g[:n], c.maps, c.mats, c.layout, c.kw, 540 + n)
    if name.startswith('clean-'):          # scene A' of the bad-input tests
        offset = float(name.split('-')[1])
        return random_case(800 + int(offset * 100), BAD_SHAPE, 8, (1, 4, 0), 2, 9, 7, 3, normal_offset=offset)
    if name.startswith('far-'):            # scene B
        return bad_scenes(float(name.split('-')[1]))[1]
    if name == 'map-5x3-inf':              # 'map-5x3' with five of its fifteen texels at +Inf or -Inf
        c = base_case('map-5x3')
        maps = c.maps.copy()
        maps.reshape(-1)[[1, 5, 6, 10, 14]] = [np.inf, -np.inf, np.inf, np.inf, -np.inf]
        return Case(c.shape, c.g, maps, c.mats, c.layout, c.kw, 550)
    if name == 'hard':
        return hard_case()
    if name.startswith('ends-'):
        return ends_case(float(name.split('-', 1)[1]))
    if name == 'image-f16':                # 'image' with maps and matrices rounded to float16
        c = base_case('image')
        return redrawn(c, c.maps.astype(np.float16).astype(np.float32), c.mats.astype(np.float16).astype(np.float32), 560)
    if name == 'image-one-matrix':         # 'image' with the first light's matrix for every light
        c = base_case('image')
        return redrawn(c, c.maps, np.stack([c.mats[0]] * 3), 570)
    raise KeyError(name)


TILE_CASES = ['many-tiles-image', 'many-tiles-flat', 'grid-3x4', 'column', 'two-rows', 'one-row']
PATCH_CASES = ['patch-offset-1', 'patch-offset-3', 'patch-offset-5', 'patch-offset-tiles', 'patch-mixed', 'patch-mixed-reversed']
FLAT_COUNTS = [1, 255, 256, 257]
RESTATED = TILE_CASES + PATCH_CASES + ['map-5x3-inf']
OTHERS = ['many-tiles-image-2', 'one-row-2', 'direct-batch-0', 'direct-batch-1', 'far-0.0', 'far-0.05', 'hard', 'image-f16', 'image-one-matrix'] \
    + ['flat-%d' % n for n in FLAT_COUNTS] + ['ends-%r' % s for s in (3.4e38, FLT_MIN)]


def tolerance_cases():
    """every case of this file that is held to the F32 table"""
    return [case(name).args for name in RESTATED + OTHERS]


# ---- where a case stands, from the float64 values of its inputs

def grid_of(c):
    rows, cols = c.shape if len(c.shape) == 2 else (1, c.shape[0])
    tw, th = (TILE, TILE) if rows > 1 else (SHADOW_BLOCK, 1)
    return rows, cols, tw, th, -(-cols // tw), -(-rows // th)


def active_lanes(c):
    """[tiles, 4]: the pixels of each wave of each backward workgroup (lane t of a tile: pixel (t // tw, t % tw) of it)"""
    rows, cols, tw, th, tiles_x, tiles_y = grid_of(c)
    t = np.arange(SHADOW_BLOCK)
    counts = np.zeros((tiles_y * tiles_x, 4), dtype=int)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            live = (tx * tw + t % tw < cols) & (ty * th + t // tw < rows)
            counts[ty * tiles_x + tx] = live.reshape(4, 64).sum(1)
    return counts


def boxes(c):
    """{(tile, light): (rmin, cmin, rows, cols) of the texels inside the map that the tile's windows hold; None: no window}, as
    the backward kernel's box_add sees them (normal_offset = 0: the designed cases)"""
    assert c.kw['normal_offset'] == 0.
    rows, cols, tw, th, tiles_x, tiles_y = grid_of(c)
    K, h = c.kw['kernel'], (c.kw['kernel'] - 1) // 2
    hs, ws = c.maps.shape[1:]
    op = c.layout[0]
    q4 = np.concatenate([c.g[:, op:op + 3].astype(np.float64), np.ones((len(c.g), 1))], 1)
    py, px = np.divmod(np.arange(rows * cols), cols)
    tile = (py // th) * tiles_x + px // tw
    res = {}
    for l, M in enumerate(c.mats.astype(np.float64)):
        x, y, _, w = (q4 @ M).T
        assert (w > 0).all()
        r0 = np.floor((1. - y / w) * hs / 2. - 0.5).astype(int) - h
        c0 = np.floor((x / w + 1.) * ws / 2. - 0.5).astype(int) - h
        on = (r0 + K >= 0) & (r0 <= hs - 1) & (c0 + K >= 0) & (c0 <= ws - 1)
        for t in range(tiles_x * tiles_y):
            sel = on & (tile == t)
            if not sel.any():
                res[t, l] = None
                continue
            rmin, rmax = max(r0[sel].min(), 0), min((r0[sel] + K).max(), hs - 1)
            cmin, cmax = max(c0[sel].min(), 0), min((c0[sel] + K).max(), ws - 1)
            res[t, l] = (int(rmin), int(cmin), int(rmax - rmin + 1), int(cmax - cmin + 1))
    return res


def stands(c, gradients=True):
    assert c.ref['kink'].min() >= R.OFF_KINKS
    if gradients:
        assert (c.ref['mass_d_maps'] > 0).any(axis=(1, 2)).all() and (c.ref['mass_d_matrices'] > 0).any(axis=(1, 2)).all()


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_the_tile_cases_stand_where_they_are_meant_to(lib):
    """The tile counts (the library's own, from the scratch it asks for), the pixels of each wave, and a gradient to every map
    and matrix: 257 tiles in a row with waves 1..3 idle, 257 tiles of a flat list with 3 pixels in the last, 3 x 4 tiles with
    partial ones on both far edges, a column (4 lanes a wave), two rows, one row (a flat list of two tiles)"""
    lanes = {}
    for name, tiles in (('many-tiles-image', 257), ('many-tiles-flat', 257), ('grid-3x4', 12), ('column', 3), ('two-rows', 2), ('one-row', 2)):
        c = case(name)
        rows, cols, tw, th, tiles_x, tiles_y = grid_of(c)
        lights = len(c.maps)
        assert tiles_x * tiles_y == tiles and lib.dirt_shadow_scratch_bytes(1, rows, cols, lights) == tiles * lights * 16 * 4, name
        lanes[name] = active_lanes(c)
        assert lanes[name].sum() == len(c.g)
        stands(c)
    assert (lanes['many-tiles-image'] == [32, 0, 0, 0]).all()
    assert lib.dirt_shadow_scratch_bytes(2, 2, 257 * TILE, 2) // (2 * 16 * 4) == 514 > 2 * 256      # shared matrices: a third turn for two lanes
    assert (lanes['many-tiles-flat'][:-1] == 64).all() and lanes['many-tiles-flat'][-1].tolist() == [3, 0, 0, 0]
    assert grid_of(case('grid-3x4'))[4:] == (4, 3) and case('grid-3x4').g.shape[1] == 9 and len(case('grid-3x4').maps) == 3
    assert lanes['grid-3x4'][3].tolist() == [8, 8, 8, 8] and lanes['grid-3x4'][8].tolist() == [48, 0, 0, 0] and lanes['grid-3x4'][11].tolist() == [6, 0, 0, 0]
    assert lanes['column'][:2].tolist() == [[4] * 4] * 2 and lanes['column'][2].tolist() == [4, 1, 0, 0]
    assert lanes['two-rows'].tolist() == [[32, 0, 0, 0], [6, 0, 0, 0]]
    assert lanes['one-row'].tolist() == [[64] * 4, [3, 0, 0, 0]]
    for name in ('many-tiles-image-2', 'one-row-2'):
        stands(case(name))


def test_the_patch_cases_stand_where_they_are_meant_to():
    """The box of every light in every tile: 'patch-offset-K' strictly inside the 64 x 56 map on all four sides and no larger than
    the LDS patch; 'patch-offset-tiles' four boxes of four origins whose neighbours share texels; 'patch-mixed' and its reverse
    a box of 41 x 41 > TEX_PATCH under the identity and smaller ones under the scaled matrices; 'direct-batch' larger than the
    patch for both lights of both scenes, each scene with texels of its own"""
    hs, ws = OFFSET_MAP
    for kernel in (1, 3, 5):
        c = case('patch-offset-%d' % kernel)
        (rmin, cmin, bh, bw), = boxes(c).values()
        assert (rmin, cmin) == (17 - (kernel - 1) // 2, 23 - (kernel - 1) // 2) and rmin > 0 and cmin > 0, kernel
        assert rmin + bh < hs and cmin + bw < ws and bw < ws and bh * bw <= TEX_PATCH and (bh, bw) == (29 + kernel, 29 + kernel), kernel
        stands(c)
    c = case('patch-offset-tiles')
    b = boxes(c)
    assert sorted(b) == [(t, 0) for t in range(4)] and len({v[:2] for v in b.values()}) == 4
    for rmin, cmin, bh, bw in b.values():
        assert rmin > 0 and cmin > 0 and rmin + bh < hs and cmin + bw < ws and bh * bw <= TEX_PATCH
    assert [b[t, 0][:2] for t in range(4)] == [(16, 22), (16, 36), (31, 22), (31, 36)]
    assert b[0, 0][1] + b[0, 0][3] > b[1, 0][1] and b[0, 0][0] + b[0, 0][2] > b[2, 0][0]           # columns, rows shared by neighbours
    stands(c)
    for name, fits in (('patch-mixed', [True, False, True]), ('patch-mixed-reversed', [False, True])):
        c = case(name)
        b = boxes(c)
        assert [b[0, l][2] * b[0, l][3] <= TEX_PATCH for l in range(len(fits))] == fits, (name, b)
        assert [b[0, l] for l in range(len(fits)) if not fits[l]] == [(0, 0, 41, 41)]
        assert c.maps.shape[1:] == (48, 48)
        stands(c)
    assert boxes(case('patch-mixed'))[0, 0] == (10, 10, 24, 24) and boxes(case('patch-mixed'))[0, 2] == (5, 5, 33, 33)
    s0, s1 = case('direct-batch-0'), case('direct-batch-1')
    assert list(boxes(s0).values()) == [(0, 0, 41, 41), (0, 0, 41, 41)] and list(boxes(s1).values()) == [(6, 6, 41, 41), (6, 6, 42, 42)]
    assert 41 * 41 > TEX_PATCH
    for a, b in ((s0, s1), (s1, s0)):
        stands(a)
        assert ((a.ref['mass_d_maps'] == 0) & (b.ref['mass_d_maps'] > 0)).any(axis=(1, 2)).all()
    for n in FLAT_COUNTS:
        stands(case('flat-%d' % n), gradients=n > 1)


# ---- the bad-input scenes

def poison_mask():
    """About one pixel in nine of the 17 x 19 image, some in every wave of every tile (one by hand in wave 0 of tile 1 and in
    tile 3, which the ninth pixels miss), and every pixel of wave 2 of tile 1 (rows 8..11 of the columns 16..18)"""
    rows, cols = BAD_SHAPE
    py, px = np.divmod(np.arange(rows * cols), cols)
    return (np.arange(rows * cols) % 9 == 4) | ((py >= 8) & (py < 12) & (px >= 16)) | ((px == 17) & ((py == 1) | (py == 16)))


def poisons(ws):
    """(x, y, z) replacements, None: the component stays"""
    nan, inf, far = float('nan'), float('inf'), 2.**33 / ws       # `far`: past 2^31 texels under the orthographic light
    return [(nan, None, None), (nan, nan, nan), (inf, None, None), (-inf, None, None), (inf, inf, inf), (3e38, None, None), (-3e38, None, None),
            (None, 1e12, None), (None, -1e12, None), (far, None, None), (-far, None, None), (None, nan, None), (None, None, -inf)]


@functools.lru_cache(maxsize=None)
def bad_scenes(offset):
    """(A, B, poisoned [N] bool): A is the clean scene with the positions of the poisoned pixels replaced by NaN, +-Inf, +-3e38,
    +-1e12 and a coordinate past 2^31 texels; B has a finite point there that is in front of every light and far off every map"""
    clean = case('clean-%s' % offset)
    op = clean.layout[0]
    poisoned = poison_mask()
    a, b = clean.g.copy(), clean.g.copy()
    kinds = poisons(clean.maps.shape[2])
    for k, i in enumerate(np.nonzero(poisoned)[0]):
        for j, x in enumerate(kinds[k % len(kinds)]):
            if x is not None:
                a[i, op + j] = x
        b[i, op:op + 3] = [8. + 0.01 * k, 0.3, -0.2] if k % 2 else [-8. - 0.01 * k, -0.4, 0.1]
    seed = 810 + int(offset * 100)
    A = Case(clean.shape, a, clean.maps, clean.mats, clean.layout, clean.kw, seed)
    return A, Case(clean.shape, b, clean.maps, clean.mats, clean.layout, clean.kw, seed), poisoned


@pytest.mark.parametrize('offset', [0., 0.05])
def test_the_bad_input_scenes_stand_where_they_are_meant_to(offset):
    """Every wave with a pixel holds a poisoned one, one wave holds nothing else, every kind of poison is used; in float64 and in
    the float32 torch form a poisoned pixel is lit by every light, and the torch form's gradients hold no NaN (+3e38 overflows
    x under the perspective light: `lighting.shadow_visibility` takes such a point as off the map before it divides); B's replacements are in front of every
    light (w > 0) with their windows off every map, and B is off the kinks"""
    A, B, poisoned = bad_scenes(offset)
    assert 0.09 < poisoned.mean() < 0.16 and poisoned.sum() >= 3 * len(poisons(7))
    rows, cols, tw, th, tiles_x, tiles_y = grid_of(A)
    py, px = np.divmod(np.arange(rows * cols), cols)
    wave = ((py // th) * tiles_x + px // tw) * 4 + ((py % th) * tw + px % tw) // 64
    waves = set(wave.tolist())
    assert waves == set(wave[poisoned].tolist()) and len(waves) == 10
    assert poisoned[wave == 4 + 2].all() and (wave == 4 + 2).sum() == 12
    op = A.layout[0]
    assert np.isfinite(np.delete(A.g, np.s_[op:op + 3], 1)).all() and not np.isfinite(A.g[poisoned, op:op + 3]).all(1).all()
    assert np.array_equal(A.g[~poisoned], B.g[~poisoned]) and np.array_equal(A.go, B.go)
    args, kw = A.args
    assert (R.compose(*args[:4], masses=False, **A.kw)['out'][poisoned] == 1.).all()      # (its hand-made chain multiplies a NaN point by 0: the value alone)
    res = R.torch_form(*args, **kw)
    assert (res['out'][poisoned] == 1.).all() and not res['d_gbuffer'][poisoned].any()
    assert all(np.isfinite(res[k]).all() for k in ('out', 'd_gbuffer', 'd_maps', 'd_matrices'))
    q = B.g[poisoned, op:op + 3].astype(np.float64)
    for M in B.mats.astype(np.float64):
        x, y, _, w = (np.concatenate([q, np.ones((len(q), 1))], 1) @ M).T
        assert (w > 0.5).all() and (np.abs(x / w) > 3.).all()      # the map ends at |x / w| = 1, the 3 x 3 window 3 texels of 2 / 7 further out
    assert (B.ref['out'][poisoned] == 1.).all() and not B.ref['d_gbuffer'][poisoned].any()
    stands(B)
    # past 2^31 texels: what no int holds
    with np.errstate(invalid='ignore'):
        x = (np.concatenate([A.g[poisoned, op:op + 3].astype(np.float64), np.ones((poisoned.sum(), 1))], 1) @ A.mats[0].astype(np.float64))[:, 0]
        assert (np.isfinite(x) & (np.abs((x + 1.) * 7 / 2.) > 2.**31)).sum() >= 8


def test_infinite_texels_stand_where_they_are_meant_to():
    """A texel at +Inf (a far plane written by hand) compares as lit, one at -Inf as shadowing, and neither gets or passes a
    gradient: the clamp's derivative is 0 there and 0 / softness is 0.  The float64 restatement and the float32 torch form hold
    no NaN and no Inf on 'map-5x3-inf', the infinite texels' gradient is an exact zero in both, and their neighbours' is not."""
    c = case('map-5x3-inf')
    inf = ~np.isfinite(c.maps)
    assert inf.sum() == 5 and (c.maps[inf] > 0).sum() == 3
    args, kw = c.args
    r32 = R.torch_form(*args, **kw)
    for res in (c.ref, r32):
        assert all(np.isfinite(res[k]).all() for k in ('out', 'd_gbuffer', 'd_maps', 'd_matrices'))
        assert not res['d_maps'][inf].any() and (res['d_maps'][~inf] != 0).all()
    assert not c.ref['mass_d_maps'][inf].any()
    assert np.array_equal(c.g, base_case('map-5x3').g) and np.abs(c.ref['out'] - base_case('map-5x3').ref['out']).max() > 0.05
    stands(c)


def test_the_hard_case_stands_where_it_is_meant_to():
    """softness 1e-6 over maps whose noise spans tenths: every window of every pixel is flat by the restatement, the value is 1
    (lit, or uncovered) or 1 - m (in the umbra: 0 where m = 1), and no point, normal, map or matrix has a gradient or a mass"""
    c = case('hard')
    ref = c.ref
    assert c.kw['softness'] == 1.e-6 and ref['flat'].all() and ref['kink'].min() >= R.OFF_KINKS
    m = c.g[:, c.layout[2]].astype(np.float64)[:, None]
    lit, umbra = ref['out'] == 1., ref['out'] == 1. - m
    assert (lit | umbra).all()
    assert (umbra & (m == 1.)).sum() >= 10 and (umbra & (m > 0.) & (m < 1.)).sum() >= 3 and (lit & (m == 1.)).sum() >= 10
    op, on, om = c.layout
    points = np.r_[op:op + 3, on:on + 3]
    assert not ref['d_maps'].any() and not ref['d_matrices'].any() and not ref['d_gbuffer'][:, points].any()
    assert not ref['mass_d_maps'].any() and ref['d_gbuffer'][:, om].any()


ENDS = (3.4e38, FLT_MIN, 1e-40)


def ends_case(softness):
    """One light, the identity matrix, an 8 x 8 map and kernel 1: twelve points at the fractions (1/4, 1/2) of their texels, in
    threes: clip z = Z + bias exactly ((Z - d) + bias is an exact 0: Z = 1/4, bias = 1/16, d = 5/16), one float32 above it, one
    below it, and 1/8 either side.  Every weight and every comparison of 0, 1/2 or 1 is a dyadic number of a few bits."""
    maps = np.full((1, 8, 8), 0.25, dtype=np.float32)
    d = np.float32(0.3125)
    depths = [d, np.nextafter(d, np.float32(1.)), np.nextafter(d, np.float32(0.)), np.float32(0.4375), np.float32(0.1875)]
    g = np.zeros((12, 3), dtype=np.float32)
    for i in range(12):
        row, col = 1 + i // 4 * 2 + 0.25, 1 + i % 4 + 0.5
        g[i] = [(col + 0.5) * 2. / 8 - 1., 1. - (row + 0.5) * 2. / 8, depths[i % 5]]
    return Case((12,), g, maps, np.eye(4, dtype=np.float32)[None], (0, None, None), dict(kernel=1, bias=0.0625, softness=softness, normal_offset=0.), 581)


def test_the_softness_ends_stand_where_they_are_meant_to():
    """(Z - d) + bias is 0, +-2^-25 (one float32 of d either side), +-1/8 in float32 as in float64; the float32 torch form gives 1/2 everywhere at
    softness 3.4e38, and 1/2, 0, 1, 0, 1 at the smallest normal float32; a softness whose float32 reciprocal is not finite
    (1e-40) is refused"""
    from dirt_amd import lighting
    c = case('ends-%r' % FLT_MIN)
    t = (c.maps[0, 0, 0] - c.g[:, 2]) + np.float32(0.0625)
    assert t.dtype == np.float32 and (t[[0, 5, 10]] == 0.).all() and sorted(set(np.abs(t).tolist())) == [0., 2.**-25, 0.125]
    args, kw = c.args
    out = R.torch_form(*args, **kw)['out'][:, 0]
    assert out.tolist() == [[0.5, 0., 1., 0., 1.][i % 5] for i in range(12)]
    args, kw = case('ends-%r' % 3.4e38).args
    assert (R.torch_form(*args, **kw)['out'] == 0.5).all()
    with pytest.raises(ValueError) as e:
        lighting.shadow_visibility(torch.zeros(1, 3), None, torch.zeros(1, 2, 2), torch.eye(4)[None], softness=1e-40)
    assert str(e.value) == 'softness must have a finite float32 reciprocal, got 1e-40'


def test_the_wrapper_cases_stand_where_they_are_meant_to():
    for name in ('image-f16', 'image-one-matrix'):
        c = case(name)
        stands(c)
        assert c.g.shape == base_case('image').g.shape
    c = case('image-f16')
    assert np.array_equal(c.maps, c.maps.astype(np.float16).astype(np.float32)) and np.array_equal(c.mats, c.mats.astype(np.float16).astype(np.float32))
    assert not np.array_equal(c.mats, base_case('image').mats)
    c = case('image-one-matrix')
    assert np.array_equal(c.mats[1], c.mats[0]) and np.array_equal(c.mats[2], c.mats[0])


# ---- GPU

@pytest.mark.gpu
@pytest.mark.parametrize('name', RESTATED)
def test_kernel_against_the_restatement(gpu, name):
    """Value and every gradient within KERNEL x F32 of the float64 restatement, massless elements exact, on the tile cases, the
    patch cases and the map with infinite texels (whose gradient must be an exact zero and no NaN anywhere)"""
    c = case(name)
    got = _run(gpu, c)
    _check(got, c, name)
    assert all(np.isfinite(got[k]).all() for k in got)


def _run_batch(gpu, scenes, shape, share_maps, share_mats):
    """A list of cases as one batch -> out [B, N, L], d_gbuffer [B, N, Cg], d_maps, d_matrices as numpy"""
    from dirt_amd import shading
    op, on, om = scenes[0].layout
    g = _dev(gpu, np.stack([s.g.reshape(shape + (-1,)) for s in scenes])).requires_grad_(True)
    Z = _dev(gpu, scenes[0].maps if share_maps else np.stack([s.maps for s in scenes])).requires_grad_(True)
    M = _dev(gpu, scenes[0].mats if share_mats else np.stack([s.mats for s in scenes])).requires_grad_(True)
    out = shading.shadow_visibility(g, Z, M, positions=op, normals=on, mask=om, **scenes[0].kw)
    assert out.shape == (len(scenes),) + shape + (len(scenes[0].maps),)
    dg, dZ, dM = (x.cpu().numpy() for x in torch.autograd.grad(out, (g, Z, M), _dev(gpu, np.stack([s.go.reshape(shape + (-1,)) for s in scenes]))))
    n = scenes[0].g.shape[0]
    return out.detach().cpu().numpy().reshape(len(scenes), n, -1), dg.reshape(len(scenes), n, -1), dZ, dM


def _total(scenes, key):
    return {key: sum(s.ref[key] for s in scenes), 'mass_' + key: sum(s.ref['mass_' + key] for s in scenes)}


def _check_batch(scenes, res, share_maps, share_mats):
    out, dg, dZ, dM = res
    for b, s in enumerate(scenes):
        _check({'out': out[b], 'd_gbuffer': dg[b], 'd_maps': None if share_maps else dZ[b], 'd_matrices': None if share_mats else dM[b]}, s, b)
    if share_maps:
        assert R.ratios({'d_maps': dZ}, _total(scenes, 'd_maps'), scenes[0].layout)['d_maps'] <= KERNEL * F32['d_maps']
        assert R.exact_where_massless({'d_maps': dZ}, _total(scenes, 'd_maps'))
    if share_mats:
        assert R.ratios({'d_matrices': dM}, _total(scenes, 'd_matrices'), scenes[0].layout)['d_matrices'] <= KERNEL * F32['d_matrices']


@pytest.mark.gpu
@pytest.mark.parametrize('share_mats', [True, False])
def test_two_scenes_of_257_tiles(gpu, share_mats):
    """[2, 2, 4112, Cg]: a shared matrix set sums 514 rows of partial sums, one per scene 257 each; the same bits on a second run"""
    scenes = [case('many-tiles-image'), case('many-tiles-image-2')]
    res = _run_batch(gpu, scenes, scenes[0].shape, True, share_mats)
    _check_batch(scenes, res, True, share_mats)
    again = _run_batch(gpu, scenes, scenes[0].shape, True, share_mats)
    assert np.array_equal(res[3], again[3]) and np.array_equal(res[1], again[1]) and np.array_equal(res[0], again[0])


@pytest.mark.gpu
def test_two_runs_of_257_tiles_give_the_same_matrix_gradient(gpu):
    c = case('many-tiles-image')
    a, b = _run(gpu, c), _run(gpu, c)
    assert np.array_equal(a['d_matrices'], b['d_matrices']) and np.array_equal(a['d_gbuffer'], b['d_gbuffer']) and np.array_equal(a['out'], b['out'])


@pytest.mark.gpu
def test_a_one_row_image_is_the_flat_list(gpu):
    """[1, 259, Cg] and [2, 1, 259, Cg] take the flat path: the bits of the call on [259, Cg] in the value, the G-buffer's and
    the matrices' gradient (per-scene matrices: each scene's own sum), the maps' within the tolerance"""
    c, c2 = case('one-row'), case('one-row-2')
    flat, flat2 = _run(gpu, c, shape=(c.g.shape[0],)), _run(gpu, c2, shape=(c.g.shape[0],))
    image = _run(gpu, c, shape=c.shape)
    _check(image, c, 'one-row')
    for k in ('out', 'd_gbuffer', 'd_matrices'):
        assert np.array_equal(image[k], flat[k]), k
    res = _run_batch(gpu, [c, c2], c.shape, True, False)
    _check_batch([c, c2], res, True, False)
    for b, f in enumerate((flat, flat2)):
        assert np.array_equal(res[0][b], f['out']) and np.array_equal(res[1][b], f['d_gbuffer']) and np.array_equal(res[3][b], f['d_matrices']), b


@pytest.mark.gpu
def test_direct_atomics_into_per_scene_maps(gpu):
    """B = 2, maps [2, 2, 48, 48], every box larger than the LDS patch: each scene's gradient lands in its own maps, and the
    texels only the other scene's windows hold stay exact zeros"""
    scenes = [case('direct-batch-0'), case('direct-batch-1')]
    res = _run_batch(gpu, scenes, scenes[0].shape, False, True)
    _check_batch(scenes, res, False, True)
    for mine, other, dZ in ((scenes[0], scenes[1], res[2][0]), (scenes[1], scenes[0], res[2][1])):
        alone = (mine.ref['mass_d_maps'] == 0) & (other.ref['mass_d_maps'] > 0)
        assert alone.any(axis=(1, 2)).all() and not dZ[alone].any()


def _c_abi(gpu, lib, c):
    """The entry points called as C would on a single scene, every output and the scratch inside a larger buffer of a guard
    value: nothing outside is written -> the keys of `compose`"""
    from dirt_amd import _lib
    rows, cols = grid_of(c)[:2]
    (hs, ws), lights, (n, cg) = c.maps.shape[1:], c.maps.shape[0], c.g.shape
    op, on, om = (-1 if x is None else x for x in c.layout)
    g, Z, M, go = (_dev(gpu, x) for x in (c.g, c.maps, c.mats, c.go))
    pad, guard = 37, -77.25
    nbytes = lib.dirt_shadow_scratch_bytes(1, rows, cols, lights)
    counts = dict(out=n * lights, d_gbuffer=n * cg, d_maps=Z.numel(), d_matrices=M.numel(), scratch=nbytes // 4)
    bufs = {k: torch.full((count + 2 * pad,), guard, dtype=torch.float32, device=gpu) for k, count in counts.items()}
    at = lambda k: bufs[k].data_ptr() + 4 * pad   # noqa: E731
    tail = (cg, op, on, om, lights, hs, ws, 1, 1, c.kw['kernel'], c.kw['bias'], c.kw['softness'], c.kw['normal_offset'], None)
    _lib.check(lib.dirt_shadow_forward(g.data_ptr(), Z.data_ptr(), M.data_ptr(), at('out'), 1, n, *tail))
    _lib.check(lib.dirt_shadow_backward(g.data_ptr(), Z.data_ptr(), M.data_ptr(), go.data_ptr(), at('d_gbuffer'), at('d_maps'), at('d_matrices'), at('scratch'),
                                        nbytes, 1, rows, cols, *tail))
    torch.cuda.synchronize()
    for k, count in counts.items():
        assert (bufs[k][:pad] == guard).all() and (bufs[k][pad + count:] == guard).all(), k
    shapes = dict(out=(n, lights), d_gbuffer=(n, cg), d_maps=c.maps.shape, d_matrices=c.mats.shape)
    return {k: bufs[k][pad:pad + counts[k]].cpu().numpy().reshape(shape) for k, shape in shapes.items()}


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['patch-past', 'patch-offset-3'] + ['flat-%d' % n for n in FLAT_COUNTS])
def test_c_abi_with_guard_values_around_every_output(gpu, lib, name):
    """Direct atomics ('patch-past'), a patch anchored off texel (0, 0), and flat lists of 1, 255, 256 and 257 pixels"""
    c = base_case(name) if name == 'patch-past' else case(name)
    _check(_c_abi(gpu, lib, c), c, name)


@pytest.mark.gpu
@pytest.mark.parametrize('offset', [0., 0.05])
def test_bad_points_are_lit_and_add_nothing(gpu, offset):
    """Scene A (NaN, +-Inf, +-3e38, +-1e12 and coordinates past 2^31 texels in one pixel of nine) against scene B (finite points
    far off the maps in their place): a poisoned pixel reads exactly 1 and its row of the gradient holds no non-zero and no NaN;
    every other row, and the matrices' gradient -- the poisoned lanes add selected zeros in the same fixed order --, are B's to
    the bit; the maps' gradient is within B's tolerance and holds no NaN"""
    A, B, poisoned = bad_scenes(offset)
    b = _run(gpu, B)
    _check(b, B, 'B')
    a = _run(gpu, A)
    assert (a['out'][poisoned] == 1.).all()
    assert not a['d_gbuffer'][poisoned].any()                  # (a NaN is non-zero)
    for k in ('out', 'd_gbuffer', 'd_matrices'):
        assert np.array_equal(a[k], b[k]), k                   # (and so finite)
    assert np.isfinite(a['d_maps']).all()
    assert R.ratios({'d_maps': a['d_maps']}, B.ref, B.layout)['d_maps'] <= KERNEL * F32['d_maps'] and R.exact_where_massless({'d_maps': a['d_maps']}, B.ref)


@pytest.mark.gpu
def test_hard_shadows_owe_exact_zeros(gpu):
    """softness 1e-6, every window flat: where the restatement says umbra (every comparison a 0) the value is 1 - m to the bit (0
    where m = 1), where it says lit it is 1 to the rounding of the window's sum (KERNEL x F32 of a mass that is at most 3);
    exact zeros to every point, normal, map and matrix; the mask's gradient within the tolerance"""
    c = case('hard')
    got = _run(gpu, c)
    _check(got, c, 'hard')
    op, on, om = c.layout
    m = np.broadcast_to(c.g[:, om:om + 1], got['out'].shape)
    umbra = c.ref['out'] == 1. - m.astype(np.float64)
    assert np.array_equal(got['out'][umbra], (np.float32(1.) - m)[umbra])
    assert (np.abs(got['out'][~umbra] - 1.) <= KERNEL * F32['out'] * 3.).all()
    assert not got['d_maps'].any() and not got['d_matrices'].any() and not got['d_gbuffer'][:, np.r_[op:op + 3, on:on + 3]].any()


@pytest.mark.gpu
@pytest.mark.parametrize('softness', ENDS[:2])
def test_the_softness_ends_against_the_float32_torch_form(gpu, softness):
    """softness 3.4e38 and the smallest normal float32, at (Z - d) + bias = 0 and one float32 either side of it: the value is the
    float32 torch form's to the bit (every term a dyadic number of a few bits: no rounding on either side), the gradients within
    the kernel's allowance plus the torch form's own (KERNEL + 1) x F32 x mass, plus the smallest normal float32 per term added
    (12 pixels x 4 texels): below it either side may flush a product to zero.  Nothing is a NaN or an Inf."""
    c = case('ends-%r' % softness)
    args, kw = c.args
    want = R.torch_form(*args, **kw)
    got = _run(gpu, c)
    assert np.array_equal(got['out'], want['out'])
    ref = c.ref
    for k in ('d_gbuffer', 'd_maps', 'd_matrices'):
        kind = {'d_gbuffer': 'd_positions'}.get(k, k)
        assert np.isfinite(got[k]).all() and np.isfinite(want[k]).all()
        excess = np.abs(got[k].astype(np.float64) - want[k]) - ((KERNEL + 1) * F32[kind] * ref['mass_' + k] + 48 * FLT_MIN)
        print(k, float(excess.max()))
        assert (excess <= 0.).all(), k


@pytest.mark.gpu
def test_a_softness_without_a_finite_reciprocal_is_refused(gpu, lib):
    """1e-40: its float32 reciprocal is Inf, and 0 x Inf at (Z - d) + bias = 0 was a NaN in the value and in every gradient.
    Refused by the wrapper and by both entry points before any device work."""
    from dirt_amd import _lib, shading
    c = ends_case(1e-40)
    g, Z, M = (_dev(gpu, x) for x in (c.g, c.maps, c.mats))
    with pytest.raises(ValueError) as e:
        shading.shadow_visibility(g, Z, M, positions=0, softness=1e-40, kernel=1, bias=0.0625)
    assert str(e.value) == 'softness must have a finite float32 reciprocal, got 1e-40'
    out = torch.full((12,), -77.25, device=gpu)
    assert lib.dirt_shadow_forward(g.data_ptr(), Z.data_ptr(), M.data_ptr(), out.data_ptr(), 1, 12, 3, 0, -1, -1, 1, 8, 8, 1, 1, 1, 0.0625, 1e-40, 0., None) \
        == _lib.E_INVALID_ARGUMENT
    assert _lib.last_error() == 'dirt_shadow_forward: softness=%g has no finite float32 reciprocal' % ctypes.c_float(1e-40).value
    torch.cuda.synchronize()
    assert (out == -77.25).all()


# ---- the wrapper

def _leaves(gpu, c, g=None, Z=None, M=None):
    return [(_dev(gpu, x) if t is None else t).requires_grad_(True) for x, t in ((c.g.reshape(c.shape + (-1,)), g), (c.maps, Z), (c.mats, M))]


def _call(c, g, Z, M):
    from dirt_amd import shading
    op, on, om = c.layout
    return shading.shadow_visibility(g, Z, M, positions=op, normals=on, mask=om, **c.kw)


def _same_layout(grad, leaf):
    assert grad.dtype == leaf.dtype and grad.shape == leaf.shape and grad.device == leaf.device


@pytest.mark.gpu
def test_float64_maps_and_matrices(gpu):
    c = base_case('image')
    dense = _run(gpu, c)
    g, Z, M = _leaves(gpu, c, Z=_dev(gpu, c.maps).double(), M=_dev(gpu, c.mats).double())
    out = _call(c, g, Z, M)
    assert out.dtype == torch.float32
    grads = torch.autograd.grad(out, (g, Z, M), _dev(gpu, c.go.reshape(c.shape + (-1,))))
    for grad, leaf in zip(grads, (g, Z, M)):
        _same_layout(grad, leaf)
    dg, dZ, dM = (x.cpu().numpy() for x in grads)
    assert np.array_equal(out.detach().cpu().numpy().reshape(dense['out'].shape), dense['out'])
    assert np.array_equal(dg.reshape(c.g.shape), dense['d_gbuffer']) and np.array_equal(dM, dense['d_matrices'].astype(np.float64))
    _check({'d_maps': dZ}, c)


@pytest.mark.gpu
def test_float16_maps_and_matrices(gpu):
    """The float32 call on the operands rounded to float16 first: the same bits in the value and the G-buffer's gradient, the
    matrices' gradient its float32 bits rounded to float16, the maps' within the tolerance plus the rounding of a float16 (half
    an ulp, 2^-11 of the value, or half the smallest subnormal, 2^-25)"""
    c = case('image-f16')
    dense = _run(gpu, c)
    _check(dense, c, 'image-f16')
    g, Z, M = _leaves(gpu, c, Z=_dev(gpu, c.maps).half(), M=_dev(gpu, c.mats).half())
    assert torch.equal(Z.float().cpu(), torch.from_numpy(c.maps)) and torch.equal(M.float().cpu(), torch.from_numpy(c.mats))
    out = _call(c, g, Z, M)
    grads = torch.autograd.grad(out, (g, Z, M), _dev(gpu, c.go.reshape(c.shape + (-1,))))
    for grad, leaf in zip(grads, (g, Z, M)):
        _same_layout(grad, leaf)
    assert np.array_equal(out.detach().cpu().numpy().reshape(dense['out'].shape), dense['out'])
    assert np.array_equal(grads[0].cpu().numpy().reshape(c.g.shape), dense['d_gbuffer'])
    assert torch.equal(grads[2].cpu(), torch.from_numpy(dense['d_matrices']).half())
    ref = c.ref
    excess = np.abs(grads[1].cpu().numpy().astype(np.float64) - ref['d_maps']) \
        - (KERNEL * F32['d_maps'] * ref['mass_d_maps'] + 2.**-11 * np.abs(ref['d_maps']) + 2.**-25)
    assert (excess <= 0.).all()


@pytest.mark.gpu
def test_maps_that_are_every_second_column_of_an_atlas(gpu):
    c = base_case('image')
    dense = _run(gpu, c)
    lights, hs, ws = c.maps.shape
    atlas = np.random.default_rng(590).uniform(-1., 1., (lights, hs, 2 * ws)).astype(np.float32)
    atlas[:, :, ::2] = c.maps
    atlas = _dev(gpu, atlas).requires_grad_(True)
    g, _, M = _leaves(gpu, c)
    Z = atlas[:, :, ::2]
    assert not Z.is_contiguous()
    out = _call(c, g, Z, M)
    grads = torch.autograd.grad(out, (g, atlas, M), _dev(gpu, c.go.reshape(c.shape + (-1,))))
    for grad, leaf in zip(grads, (g, atlas, M)):
        _same_layout(grad, leaf)
    dg, dA, dM = (x.cpu().numpy() for x in grads)
    assert np.array_equal(out.detach().cpu().numpy().reshape(dense['out'].shape), dense['out'])
    assert np.array_equal(dg.reshape(c.g.shape), dense['d_gbuffer']) and np.array_equal(dM, dense['d_matrices'])
    assert not dA[:, :, 1::2].any()
    _check({'d_maps': dA[:, :, ::2]}, c)


@pytest.mark.gpu
def test_one_matrix_expanded_to_every_light(gpu):
    """A [4, 4] leaf expanded to [3, 4, 4] (stride 0): the bits of the dense call in the value and the G-buffer's gradient; the
    leaf's gradient is the sum over the lights of the dense call's -- three float32 terms, which any order of adding gives to two
    roundings of a partial sum, 2^-23 of the sum of their absolute values"""
    c = case('image-one-matrix')
    dense = _run(gpu, c)
    _check(dense, c, 'image-one-matrix')
    leaf = _dev(gpu, c.mats[0]).requires_grad_(True)
    M = leaf.expand(3, 4, 4)
    assert M.stride(0) == 0
    g, Z, _ = _leaves(gpu, c)
    out = _call(c, g, Z, M)
    grads = torch.autograd.grad(out, (g, Z, leaf), _dev(gpu, c.go.reshape(c.shape + (-1,))))
    for grad, x in zip(grads, (g, Z, leaf)):
        _same_layout(grad, x)
    dg, dZ, dM = (x.cpu().numpy() for x in grads)
    assert np.array_equal(out.detach().cpu().numpy().reshape(dense['out'].shape), dense['out'])
    assert np.array_equal(dg.reshape(c.g.shape), dense['d_gbuffer'])
    total = dense['d_matrices'].astype(np.float64)
    assert (np.abs(dM - total.sum(0)) <= 2.**-23 * np.abs(total).sum(0)).all() and dM.any()
    _check({'d_maps': dZ}, c)


@pytest.mark.gpu
def test_a_gbuffer_that_is_a_channel_slice(gpu):
    c = base_case('image')
    dense = _run(gpu, c)
    cg = c.g.shape[1]
    wide = np.random.default_rng(591).standard_normal(c.shape + (cg + 8,)).astype(np.float32)
    wide[..., 3:3 + cg] = c.g.reshape(c.shape + (-1,))
    wide = _dev(gpu, wide).requires_grad_(True)
    _, Z, M = _leaves(gpu, c)
    g = wide[..., 3:3 + cg]
    assert not g.is_contiguous()
    out = _call(c, g, Z, M)
    grads = torch.autograd.grad(out, (wide, Z, M), _dev(gpu, c.go.reshape(c.shape + (-1,))))
    for grad, leaf in zip(grads, (wide, Z, M)):
        _same_layout(grad, leaf)
    dW, dZ, dM = (x.cpu().numpy() for x in grads)
    assert np.array_equal(out.detach().cpu().numpy().reshape(dense['out'].shape), dense['out'])
    assert np.array_equal(dW[..., 3:3 + cg].reshape(c.g.shape), dense['d_gbuffer']) and np.array_equal(dM, dense['d_matrices'])
    assert not dW[..., :3].any() and not dW[..., 3 + cg:].any()
    _check({'d_maps': dZ}, c)


@pytest.mark.gpu
def test_a_second_backward_doubles_the_gradients(gpu):
    """retain_graph=True: the entry point clears grad_maps itself on each call, and autograd adds the two results: twice the
    first to the bit for the G-buffer and the matrices, within the tolerance for the maps (x / 2 is exact)"""
    c = base_case('image')
    g, Z, M = _leaves(gpu, c)
    out = _call(c, g, Z, M)
    go = _dev(gpu, c.go.reshape(c.shape + (-1,)))
    out.backward(go, retain_graph=True)
    first = [x.grad.clone() for x in (g, Z, M)]
    _check({'d_gbuffer': first[0].cpu().numpy().reshape(c.g.shape), 'd_maps': first[1].cpu().numpy(), 'd_matrices': first[2].cpu().numpy()}, c)
    out.backward(go)
    assert torch.equal(g.grad, 2. * first[0]) and torch.equal(M.grad, 2. * first[2])
    _check({'d_maps': (Z.grad / 2.).cpu().numpy()}, c)
