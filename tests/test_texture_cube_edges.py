"""The cube-map look-up (dirt_texture_cube.hip) where tests/test_texture_cube.py stops: the forward's grid-stride loop on its second
turn, through each of its three `continue`s; the C entry points between guard values with the backward run as an image whose tiles
at the right and bottom edge are partial, and with strides wider than the data; and four channels through both the float4 kernel
and -- from pointers that are not 16-byte aligned, which no torch tensor has -- the generic one.  The reference, the tolerance and
the helpers are test_texture_cube.py's."""
import numpy as np
import pytest
import torch

from tests import cube_reference as cr
from tests.test_texture_cube import SENTINEL, TOL, _dev, _per_element, dirs_from_indices, random_dirs

GRID_LANES = 16384 * 256     # `capped_blocks`: a grid-stride launch has at most 16 384 workgroups of 256 lanes
PERIOD = 4099                # a prime: no lane meets the same table row twice
INVALID = np.array([[0, 0, 0], [np.nan, 1, 0], [1, np.inf, 0], [0, 2, -np.inf], [-0., 0, -0.], [np.nan, np.nan, np.nan]], np.float32)


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import build, _lib
    build.build_library()
    return _lib.load()


def _tables(rng, levels):
    """4 099 directions, one in twenty invalid (zeros, NaN, Inf), and as many levels of detail: every fifth an exact integer
    (f == 0), the rest fractions, values below 0 and above levels - 1, and NaN."""
    d = random_dirs(rng, (PERIOD,))
    bad = rng.choice(PERIOD, PERIOD // 20, replace=False)
    d[bad] = INVALID[np.arange(len(bad)) % len(INVALID)]
    lod = rng.uniform(-1., levels + 0.5, PERIOD).astype(np.float32)
    lod[::5] = np.arange(len(lod[::5])) % levels
    lod[3::41] = np.nan
    return d, lod


@pytest.mark.gpu
@pytest.mark.parametrize('ct,filt', [(1, 'bilinear'), (1, 'nearest'), (3, 'nearest'), (4, 'bilinear'), (3, 'trilinear')])
def test_forward_past_the_grid_cap(gpu, ct, filt):
    """4 194 304 + 300 flat look-ups into a cube of 8: the last 300 are the second turn of the forward's grid-stride loop, and
    among them are invalid directions, 'nearest' look-ups and trilinear ones with f == 0 -- the loop's three `continue`s -- as
    well as look-ups that run to its end.  Directions (and levels of detail) repeat tables of 4 099 rows, so the reference runs on
    the tables: the first 4 099 outputs against it (TOL of the blend's magnitude; 'nearest' exact), every output i the bits of
    output i % 4 099, invalid rows exactly 0."""
    from dirt_amd import texture
    rng = np.random.default_rng(300)
    size, levels = 8, 4
    n = GRID_LANES + 300
    cube = rng.uniform(-1, 1, (6, size, size, ct)).astype(np.float32)
    d, lod = _tables(rng, levels)
    if filt != 'trilinear':
        lod = None
    valid = cr.Look(d).valid
    second = (GRID_LANES + np.arange(300)) % PERIOD     # the table rows of the second turn
    assert 0.04 < 1. - valid.mean() < 0.08 and (~valid[second]).sum() >= 5 and valid[second].sum() >= 200
    if lod is not None:
        with np.errstate(invalid='ignore'):
            whole, part = valid & (lod == np.floor(lod)) & (lod >= 0) & (lod <= levels - 1), valid & (lod != np.floor(lod)) & (lod > 0) & (lod < levels - 1)
        assert whole[second].sum() >= 20 and part[second].sum() >= 20 and np.isnan(lod[second]).any()
        assert (lod[valid] < 0).any() and (lod[valid] > levels - 1).any()
    which = torch.arange(n, device=gpu) % PERIOD
    out = texture.sample_texture_cube(_dev(gpu, cube), _dev(gpu, d)[which], filt, lod=None if lod is None else _dev(gpu, lod)[which])
    assert out.shape == (n, ct)
    want, mag = cr.sample(cube, d, filt, lod=lod, magnitude=True)
    head = out[:PERIOD]
    if filt == 'nearest':
        assert np.array_equal(head.cpu().numpy().view(np.uint32), want.view(np.uint32)), "'nearest' is exact"
    else:
        _per_element(head, want, mag, 'past the grid cap C=%d %s' % (ct, filt))
    assert not head.cpu().numpy()[~valid].any() and bool(head[_dev(gpu, valid)].any())
    assert torch.equal(out.view(torch.int32), head.view(torch.int32)[which]), 'an output differs from the one of the same table row'


# ---- through the C ABI --------------------------------------------------------------------------------------------------

H, W = 19, 35     # two rows and three columns of 16 x 16 tiles: the right ones 3 pixels wide, the bottom ones 3 pixels high
PAD = 64          # guard floats on each side: 256 bytes, so that an aligned allocation stays aligned behind them


def _image(rng, levels):
    """Directions [19, 35, 3] and levels of detail [19, 35]: the tiles of columns 0..15 random (every face in a tile: straight to
    memory), those of columns 16..34 -- the partial ones at the right among them -- a smooth field on face +Y at nearly one
    level (the LDS patch), both with invalid directions among them."""
    d = random_dirs(rng, (H, W))
    py, px = np.meshgrid(np.arange(float(H)), np.arange(float(W - 16)), indexing='ij')
    d[:, 16:] = dirs_from_indices(2, 1. + 0.2 * py, 2. + 0.15 * px, 8, 1.5)
    d[4, 20], d[17, 33], d[18, 34], d[18, 0] = INVALID[:4]
    lod = rng.uniform(-0.5, levels - 0.5, (H, W)).astype(np.float32)
    lod[:, 16:] = 1.25 + 0.01 * px
    lod[2, 18], lod[18, 30], lod[0, 16] = np.nan, 2.0, -1.0
    q = cr.Look(d)
    face, valid = q.face.reshape(H, W), q.valid.reshape(H, W)
    assert set(face[:, 16:][valid[:, 16:]]) == {2} and len(set(face[:16, :16][valid[:16, :16]])) == 6 and len(set(face[16:, :16][valid[16:, :16]])) >= 4
    return d, lod


def _through_the_abi(gpu, lib, cube, d, g, lod, shift=0):
    """dirt_texture_cube_forward as a flat list and _backward as the H x W image, every output between PAD guard floats: the
    directions in channels 4..6 of a G-buffer [H * W, 10] (dir_stride 10), grad_directions five floats apart.  `shift`: floats by
    which out, grad_out and the pyramid are moved off their 16-byte alignment.  Checks the guards and the floats between the
    gradient's rows, and every value against the reference.  -> (out, grad_pyramid, grad_directions, grad_lod, pointers) on the CPU"""
    from dirt_amd import rasterise_ops as ops, texture
    size, ct, n = cube.shape[1], cube.shape[3], H * W
    levels = 4 if lod is not None else 1
    filt = 'trilinear' if lod is not None else 'bilinear'
    pyr = torch.stack([torch.cat([lv.reshape(-1) for lv in texture.mip_pyramid(_dev(gpu, cube[f]))]) for f in range(6)]) if levels > 1 else _dev(gpu, cube).reshape(6, -1)
    floats = pyr.shape[1]
    stream = ops._stream_handle(gpu)

    def moved(t):     # a copy of t `shift` floats into a fresh buffer -> (the buffer, which keeps it alive; the copy's address)
        buf = torch.zeros(shift + t.numel(), device=gpu)
        buf[shift:] = t.reshape(-1)
        return buf, buf.data_ptr() + 4 * shift

    def guarded(count, off=0):
        buf = torch.full((PAD + off + count + PAD,), SENTINEL, device=gpu)
        return buf, buf.data_ptr() + 4 * (PAD + off), buf[PAD + off:PAD + off + count]

    def guards_kept(buf, off=0):
        return bool((buf[:PAD + off] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all())

    pyr_buf, pyr_ptr = moved(pyr)
    gout_buf, gout_ptr = moved(_dev(gpu, g))
    gbuf = torch.randn(n, 10, device=gpu)
    gbuf[:, 4:7] = _dev(gpu, d).reshape(n, 3)
    d_ptr = gbuf.data_ptr() + 4 * 4
    l_t = _dev(gpu, lod).reshape(n) if lod is not None else None
    l_ptr = l_t.data_ptr() if l_t is not None else None
    out_buf, out_ptr, out = guarded(n * ct, shift)
    gpyr_buf, gpyr_ptr, gpyr = guarded(6 * floats)
    gpyr[:] = float('nan')     # handed over full of garbage: comes back as the gradient alone
    gpyr[::3] = 1e30
    gdir_buf, gdir_ptr, gdir = guarded(n * 5)
    glod_buf, glod_ptr, glod = guarded(n)
    assert lib.dirt_texture_cube_forward(pyr_ptr, d_ptr, l_ptr, out_ptr, n, size, ct, levels, 10, 0.0, 0, stream) == 0, lib.dirt_texture_last_error()
    assert lib.dirt_texture_cube_backward(pyr_ptr, d_ptr, l_ptr, gout_ptr, gpyr_ptr, gdir_ptr, glod_ptr if lod is not None else None, H, W, size, ct, levels,
                                          10, 5, 0.0, 0, stream) == 0, lib.dirt_texture_last_error()
    torch.cuda.synchronize()
    assert guards_kept(out_buf, shift) and guards_kept(gpyr_buf) and guards_kept(gdir_buf) and guards_kept(glod_buf)
    rows = gdir.view(n, 5)
    assert bool((rows[:, 3:] == SENTINEL).all()), 'the two floats between the rows of grad_directions'
    assert lod is not None or bool((glod_buf == SENTINEL).all())
    got_pyr = gpyr.view(6, floats)
    if levels > 1:
        collapsed = torch.empty(6, size, size, ct, device=gpu)
        assert lib.dirt_texture_mip_collapse_batch(got_pyr.contiguous().data_ptr(), collapsed.data_ptr(), 6, size, size, ct, levels, stream) == 0
        torch.cuda.synchronize()
        got_pyr = collapsed
    what = 'C=%d %s shift %d' % (ct, filt, shift)
    want, mag = cr.sample(cube, d, filt, lod=lod, magnitude=True)
    r = cr.grad(cube, d, g, filt, lod=lod)
    bad = ~cr.Look(d).valid
    res = [x.cpu().numpy().copy() for x in (out.view(H, W, ct), got_pyr.reshape(6, size, size, ct), rows[:, :3].reshape(H, W, 3), glod.view(H, W))]
    _per_element(res[0], want, mag, what + ' forward')
    _per_element(res[1], r['grad_cube'], r['mass_cube'], what + ' grad_pyramid')
    _per_element(res[2], r['grad_directions'], r['mass_directions'], what + ' grad_directions')
    assert not res[0].reshape(n, ct)[bad].any() and not res[2].reshape(n, 3)[bad].any()
    if lod is not None:
        _per_element(res[3], r['grad_lod'], r['mass_lod'], what + ' grad_lod')
        assert not res[3].reshape(n)[bad].any()
    return res + [(pyr_ptr, gout_ptr, out_ptr, gpyr_ptr)]


@pytest.mark.gpu
@pytest.mark.parametrize('filt', ['bilinear', 'trilinear'])
@pytest.mark.parametrize('ct', [1, 4, 5])
def test_c_abi_as_an_image_with_partial_tiles_between_guards(gpu, lib, ct, filt):
    """The backward on 19 x 35 pixels (tiles of 16 x 16: 3 pixels wide at the right edge, 3 high at the bottom) with
    grad_dir_stride 5, the forward with dir_stride 10, N = 8 with 4 levels when trilinear: nothing outside out, grad_pyramid,
    grad_directions (nor between its rows) and grad_lod is written, and every value is the reference's."""
    rng = np.random.default_rng(310 + ct)
    cube = rng.uniform(-1, 1, (6, 8, 8, ct)).astype(np.float32)
    d, lod = _image(rng, 4)
    g = rng.standard_normal((H, W, ct)).astype(np.float32)
    _through_the_abi(gpu, lib, cube, d, g, lod if filt == 'trilinear' else None)


@pytest.mark.gpu
@pytest.mark.parametrize('filt', ['bilinear', 'trilinear'])
def test_four_channels_through_the_float4_kernels_and_the_generic_ones(gpu, lib, filt):
    """`dispatch_channels` takes the generic kernel at four channels when a pointer it would access as float4 is not 16-byte
    aligned -- which Python cannot hand over.  Once with every pointer aligned (asserted), once with out, grad_out and the
    pyramid one float into their buffers: both match the reference (inside `_through_the_abi`).  Whether the two agree bit for
    bit is printed, not asserted: nothing promises it.  (On an MI355X out, grad_directions and grad_lod had the same bits;
    grad_pyramid, summed by float atomics in an order that changes from run to run, had not.)"""
    rng = np.random.default_rng(320)
    cube = rng.uniform(-1, 1, (6, 8, 8, 4)).astype(np.float32)
    d, lod = _image(rng, 4)
    g = rng.standard_normal((H, W, 4)).astype(np.float32)
    lod = lod if filt == 'trilinear' else None
    aligned = _through_the_abi(gpu, lib, cube, d, g, lod)
    assert all(p % 16 == 0 for p in aligned[4]), aligned[4]
    moved = _through_the_abi(gpu, lib, cube, d, g, lod, shift=1)
    assert all(p % 16 == 4 for p in moved[4][:3]), moved[4]
    names = ('out', 'grad_pyramid', 'grad_directions', 'grad_lod')[:4 if lod is not None else 3]
    print(filt, ' '.join('%s: %s' % (k, 'same bits' if np.array_equal(a.view(np.uint32), b.view(np.uint32)) else 'bits differ')
                         for k, a, b in zip(names, aligned, moved)))
