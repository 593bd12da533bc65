"""The nearest / bilinear look-up (dirt_texture.hip) where tests/test_texture.py does not reach: the three C entry points
driven through ctypes (refusals, NULL grad_uvs, strides, the flat-list entry point), guard values around every output, the
sizes where the kernels' loop, grid and LDS patch turn over, every branch of the pair-load test and of the alignment
dispatch, the wrapper's conversions, streams and graph capture, and float32 denormals.  The reference is
oracle/texture_oracle.py throughout: the forward bit for bit, gradients per element by the mass of their terms."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import texture_oracle as tex_oracle
from tests.test_texture import _forward_equal, _per_element, _smooth_uv

SENTINEL = 123.0
GUARD = 64          # guard floats on each side of an output (a multiple of 4: the operand keeps its buffer's 16-byte alignment)
TEX_PATCH = 1600    # dirt_texture.hip: the texels of a tile's LDS patch
FWD, BWD = 'dirt_texture_sample_forward', 'dirt_texture_sample_backward'   # the names the entry points report under
MODES = ('repeat', 'clamp')
FILTERS = ('bilinear', 'nearest')


@pytest.fixture(scope='module')
def lib():
    from dirt_amd import build, _lib
    build.build_library()
    return _lib.load()


def _flags(mode, filt):
    from dirt_amd import _lib
    return {'repeat': 0, 'clamp': _lib.TEX_CLAMP}[mode] | {'bilinear': 0, 'nearest': _lib.TEX_NEAREST}[filt]


# ---- the C entry points' argument checks, before any device work (CPU) ------------------------------------------------

def test_entry_points_refuse_bad_arguments_before_any_device_work(lib):
    """Every refusal of the three entry points: the return code and the full text of dirt_texture_last_error().  A refused
    call never reaches the device, so the pointers are arbitrary non-NULL values; this machine needs no GPU."""
    from dirt_amd import _lib
    p = ctypes.c_void_p(16)     # never dereferenced: validation fails first
    err = lib.dirt_texture_last_error

    def fwd(tex=p, uvs=p, out=p, n=4, ht=8, wt=8, ct=3, uv_stride=2, flags=0):
        return lib.dirt_texture_sample_forward(tex, uvs, out, n, ht, wt, ct, uv_stride, flags, None)

    def img(tex=p, uvs=p, gout=p, gtex=p, guv=p, rows=2, cols=2, ht=8, wt=8, ct=3, uv_stride=2, guv_stride=2, flags=0):
        return lib.dirt_texture_sample_backward_image(tex, uvs, gout, gtex, guv, rows, cols, ht, wt, ct, uv_stride, guv_stride, flags, None)

    def flat(tex=p, uvs=p, gout=p, gtex=p, guv=p, n=4, ht=8, wt=8, ct=3, uv_stride=2, guv_stride=2, flags=0):
        return lib.dirt_texture_sample_backward(tex, uvs, gout, gtex, guv, n, ht, wt, ct, uv_stride, guv_stride, flags, None)

    def refused(rc, text):
        assert rc == _lib.E_INVALID_ARGUMENT, (rc, text, err())
        assert err() == text.encode(), (text, err())

    sizes = '%s: bad sizes (n=%d Ht=%d Wt=%d Ct=%d uv_stride=%d)'
    for call, who in ((fwd, FWD), (img, BWD), (flat, BWD)):   # (the flat entry point reports under the image one's name)
        for (ht, wt, ct) in ((0, 8, 3), (8, 0, 3), (8, 8, 0), (-1, 8, 3), (8, -5, 3), (8, 8, -2)):
            refused(call(ht=ht, wt=wt, ct=ct), sizes % (who, 4, ht, wt, ct, 2))
        for stride in (1, 0, -2):
            refused(call(uv_stride=stride), sizes % (who, 4, 8, 8, 3, stride))
        refused(call(tex=None), '%s: texture / uvs is NULL' % who)
        refused(call(uvs=None), '%s: texture / uvs is NULL' % who)
    refused(fwd(n=-1), sizes % (FWD, -1, 8, 8, 3, 2))
    refused(fwd(out=None), FWD + ': out is NULL')
    grid = BWD + ': bad pixel grid (rows=%d cols=%d)'
    refused(img(rows=-1), grid % (-1, 2))
    refused(img(cols=-3), grid % (2, -3))
    refused(img(rows=-1, cols=-1), grid % (-1, -1))
    refused(flat(n=-1), grid % (1, -1))
    refused(img(rows=1 << 32, cols=1 << 32), grid % (1 << 32, 1 << 32))                    # rows * cols = 2^64
    refused(img(rows=3, cols=(1 << 62)), grid % (3, 1 << 62))                              # ... just past 2^63 - 1
    for call in (img, flat):
        refused(call(gout=None), BWD + ': grad_out / grad_texture is NULL')
        refused(call(gtex=None), BWD + ': grad_out / grad_texture is NULL')
        for stride in (1, 0, -2):
            refused(call(guv_stride=stride), BWD + ': grad_uv_stride < 2')
    # the order of the checks: the pixel grid, the sizes, texture / uvs, grad_out / grad_texture, grad_uv_stride
    refused(img(rows=-1, ht=0, tex=None), grid % (-1, 2))
    refused(img(ht=0, tex=None, gout=None), sizes % (BWD, 4, 0, 8, 3, 2))
    refused(img(tex=None, gout=None, guv_stride=1), BWD + ': texture / uvs is NULL')
    refused(img(gout=None, guv_stride=1), BWD + ': grad_out / grad_texture is NULL')

    # what is NOT refused: no look-ups, with every pointer NULL; and a grad_uv_stride nobody reads (grad_uvs NULL)
    def accepted(rc):
        assert rc == 0 and err() == b'', (rc, err())

    accepted(fwd(tex=None, uvs=None, out=None, n=0))
    accepted(flat(tex=None, uvs=None, gout=None, gtex=None, guv=None, n=0))
    accepted(img(tex=None, uvs=None, gout=None, gtex=None, guv=None, rows=0, cols=5))
    accepted(img(tex=None, uvs=None, gout=None, gtex=None, guv=None, rows=5, cols=0))
    accepted(img(tex=None, uvs=None, gout=None, gtex=None, guv=None, rows=0, cols=0, guv_stride=0))
    refused(img(tex=None, uvs=None, gout=None, gtex=None, guv=None, rows=0, cols=0, ht=0), sizes % (BWD, 0, 0, 8, 3, 2))
    refused(fwd(tex=None, uvs=None, out=None, n=0, uv_stride=1), sizes % (FWD, 0, 8, 8, 3, 1))


# ---- the backward kernel's tile decision, restated (CPU) --------------------------------------------------------------

def _tile_boxes(uv, ht, wt, mode, filt, rows, cols):
    """(bh, bw) of the bounding box of the taps of every tile of the backward kernel, [tiles_y, tiles_x, 2]: tiles of
    16 x 16 pixels of the rows x cols grid, 256 x 1 where rows == 1.  The taps are the oracle's: the four of
    texture_oracle._taps, or the one truncated index of 'nearest'.  A tile sums in its LDS patch iff bh * bw <= TEX_PATCH."""
    idx = tex_oracle._indices(np.asarray(uv, np.float32).reshape(-1, 2), ht, wt, mode)
    assert idx.shape[0] == rows * cols
    if filt == 'nearest':
        r0 = r1 = np.clip(tex_oracle._int(idx[:, 0]), 0, ht - 1)
        c0 = c1 = np.clip(tex_oracle._int(idx[:, 1]), 0, wt - 1)
    else:
        r0, r1, c0, c1, _, _ = tex_oracle._taps(idx.astype(np.float64), ht, wt)
    tw, th = (16, 16) if rows > 1 else (256, 1)
    pix = np.arange(rows * cols).reshape(rows, cols)
    out = np.zeros(((rows + th - 1) // th, (cols + tw - 1) // tw, 2), np.int64)
    for ty in range(out.shape[0]):
        for tx in range(out.shape[1]):
            sel = pix[th * ty:th * ty + th, tw * tx:tw * tx + tw].reshape(-1)
            out[ty, tx] = (r1[sel].max() - r0[sel].min() + 1, c1[sel].max() - c0[sel].min() + 1)
    return out


def test_tile_boxes_on_hand_made_cases():
    one = np.array([[0.3, 0.6]], np.float32)                                  # index (row 4.8, column 2.4) of 8 x 8
    assert _tile_boxes(one, 8, 8, 'repeat', 'bilinear', 1, 1).tolist() == [[[2, 2]]]
    assert _tile_boxes(one, 8, 8, 'clamp', 'nearest', 1, 1).tolist() == [[[1, 1]]]
    last = np.array([[7.5 / 8, 7.25 / 8]], np.float32)                        # inside the last texel: r1 == r0, c1 == c0
    assert _tile_boxes(last, 8, 8, 'repeat', 'bilinear', 1, 1).tolist() == [[[1, 1]]]
    assert _tile_boxes(np.array([[1.0, 0.3]], np.float32), 8, 8, 'clamp', 'bilinear', 1, 1).tolist() == [[[2, 1]]]
    seam = np.array([[-0.01, 0.3], [0.01, 0.3]], np.float32)                   # columns 7 and 0..1 in 'repeat': the whole width
    assert _tile_boxes(seam, 8, 8, 'repeat', 'bilinear', 1, 2).tolist() == [[[2, 8]]]
    assert _tile_boxes(seam, 8, 8, 'clamp', 'bilinear', 1, 2).tolist() == [[[2, 2]]]
    assert _tile_boxes(seam, 8, 8, 'repeat', 'nearest', 1, 2).tolist() == [[[1, 8]]]
    # tiles: 16 x 16 of an image, 256 x 1 of a flat list (rows == 1), partial tiles at the ends
    ys, xs = np.meshgrid(np.arange(17.), np.arange(33.), indexing='ij')
    uv = np.stack([(0.25 + xs) / 64, (0.25 + 2 * ys) / 64], -1).astype(np.float32)
    assert _tile_boxes(uv, 64, 64, 'repeat', 'bilinear', 17, 33).tolist() == [[[32, 17], [32, 17], [32, 2]], [[2, 17], [2, 17], [2, 2]]]
    assert _tile_boxes(uv, 64, 64, 'repeat', 'nearest', 17, 33)[0].tolist() == [[31, 16], [31, 16], [31, 1]]
    flat = np.stack([(0.25 + np.arange(300.) / 10) / 64, np.full(300, 0.5)], -1).astype(np.float32)
    assert _tile_boxes(flat, 64, 64, 'clamp', 'bilinear', 1, 300).tolist() == [[[2, 27], [2, 7]]]


def test_the_oracle_keeps_float32_denormals():
    """The reference of the denormal tests below must not flush: a denormal texel, coordinate and grad_out come through."""
    tiny = np.float32(2.0 ** -140)
    tex = np.full((2, 2, 1), tiny, np.float32)
    assert tex_oracle.sample_texture_uv(tex, np.array([[0.25, 0.25]], np.float32))[0, 0] == tiny
    assert tex_oracle.sample_texture_uv(np.arange(4, dtype=np.float32).reshape(2, 2, 1), np.array([[-1e-40, 0.0]], np.float32))[0, 0] == 1.0
    gt, _ = tex_oracle.sample_texture_uv_grad(tex, np.array([[0.25, 0.25]], np.float32), np.array([[tiny]], np.float32))
    assert gt[0, 0, 0] == tiny * np.float32(0.25) and gt[0, 0, 0] != 0


# ---- helpers of the GPU tests -----------------------------------------------------------------------------------------

def _dev(gpu, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _check_grads(gt, guv, tex, uv, g, mode, filt, what):
    """grad_texture (and grad_uvs, unless None) per element against the oracle's, by the mass of each element's terms."""
    want_t, want_uv, mt, muv = tex_oracle.sample_texture_uv_grad(tex, uv, g, mode, filt, want_mass=True)
    _per_element(gt.reshape(tex.shape), want_t, mt, what + ' grad_texture')
    if guv is not None:
        _per_element(guv.reshape(want_uv.shape), want_uv, muv, what + ' grad_uvs')


def _lookup(gpu, tex, uv, g, mode, filt, what):
    """Through the wrapper: forward bit for bit, both gradients per element."""
    from dirt_amd import texture
    t, u = _dev(gpu, tex).requires_grad_(True), _dev(gpu, uv).requires_grad_(True)
    out = texture.sample_texture_uv(t, u, mode, filt)
    _forward_equal(out, tex_oracle.sample_texture_uv(tex, uv, mode, filt), what + ' forward')
    gt, gu = torch.autograd.grad(out, [t, u], _dev(gpu, g))
    _check_grads(gt, gu, tex, uv, g, mode, filt, what)


def _at_end(gpu, a, lead=GUARD):
    """`a` flat, flush against the END of a buffer of its own (lead + a.size floats) -> the operand."""
    buf = torch.zeros(lead + a.size, device=gpu)
    buf[lead:] = _dev(gpu, a.reshape(-1))
    return buf[lead:]


def _guarded(gpu, size):
    """An output of `size` floats with GUARD sentinel floats on both sides, itself filled with the sentinel -> (buffer, operand)."""
    buf = torch.full((GUARD + size + GUARD,), SENTINEL, device=gpu)
    return buf, buf[GUARD:GUARD + size]


def _guards_intact(buf, size):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + size:] == SENTINEL).all())


class _C:
    """The three entry points on device tensors (any operand may be a tensor, an address or None)."""

    def __init__(self, lib, gpu, tex_shape, mode, filt):
        from dirt_amd import rasterise_ops as ops
        self.lib, self.shape, self.flags, self.stream = lib, tuple(int(d) for d in tex_shape), _flags(mode, filt), ops._stream_handle(gpu)

    @staticmethod
    def _p(x):
        return x.data_ptr() if isinstance(x, torch.Tensor) else x

    def _done(self, rc):
        assert rc == 0, (rc, self.lib.dirt_texture_last_error())
        torch.cuda.synchronize()

    def forward(self, tex, uvs, out, n, uv_stride=2):
        self._done(self.lib.dirt_texture_sample_forward(self._p(tex), self._p(uvs), self._p(out), n, *self.shape, uv_stride, self.flags, self.stream))

    def backward_image(self, tex, uvs, gout, gtex, guv, rows, cols, uv_stride=2, guv_stride=2):
        self._done(self.lib.dirt_texture_sample_backward_image(self._p(tex), self._p(uvs), self._p(gout), self._p(gtex), self._p(guv), rows, cols,
                                                               *self.shape, uv_stride, guv_stride, self.flags, self.stream))

    def backward(self, tex, uvs, gout, gtex, guv, n, uv_stride=2, guv_stride=2):
        self._done(self.lib.dirt_texture_sample_backward(self._p(tex), self._p(uvs), self._p(gout), self._p(gtex), self._p(guv), n,
                                                         *self.shape, uv_stride, guv_stride, self.flags, self.stream))


# ---- the LDS patch at its size limit ----------------------------------------------------------------------------------

def _affine_tile(dr, dc, wt=128):
    """One 16 x 16 tile over a 128 x 128 texture: row index 20.25 + dr * y / 15, column index 20.25 + dc * x / 15."""
    ys, xs = np.meshgrid(np.arange(16.), np.arange(16.), indexing='ij')
    return np.stack([(20.25 + dc * xs / 15) / wt, (20.25 + dr * ys / 15) / wt], -1).astype(np.float32)


# (span of the row index, span of the column index) over the tile -> the box of its taps: bilinear taps floor(20.25) = 20 to
# floor(20.25 + d) + 1, i.e. floor(20.25 + d) - 18 texels; the one tap of 'nearest' floor(20.25 + d) - 19
_BILINEAR_BOXES = (((38.25, 38.25), (40, 40)), ((23.25, 62.25), (25, 64)), ((62.25, 23.25), (64, 25)),      # exactly 1 600
                   ((39.0, 38.25), (41, 40)), ((16.05, 87.0), (18, 89)))                                    # 1 640, 1 602
_NEAREST_BOXES = (((39.0, 39.0), (40, 40)), ((24.0, 63.0), (25, 64)), ((63.0, 24.0), (64, 25)), ((40.5, 39.0), (41, 40)))


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 5, 8])
def test_patch_of_exactly_1600_texels_and_the_first_sizes_past_it(gpu, ct):
    """dirt_texture.hip's own `bh * bw <= TEX_PATCH`, s_acc and patch indexing: boxes of exactly 1 600 texels in three
    aspect ratios (the LDS patch, full to its last float) and the first sizes past it (global atomics), for the 1-, 3-
    and 4-channel kernels and the generic one's passes of four channels (5, 8), in both modes; 'nearest' with its
    one-tap box.  _tile_boxes asserts that every input sits where its name says; both paths meet the same tolerance."""
    rng = np.random.default_rng(50 + ct)
    tex = rng.uniform(-1, 1, (128, 128, ct)).astype(np.float32)
    g = rng.standard_normal((16, 16, ct)).astype(np.float32)
    sizes = set()
    for filt, cases in (('bilinear', _BILINEAR_BOXES), ('nearest', _NEAREST_BOXES)):
        for (dr, dc), box in cases:
            uv = _affine_tile(dr, dc)
            for mode in MODES:
                assert _tile_boxes(uv, 128, 128, mode, filt, 16, 16).tolist() == [[list(box)]]
                _lookup(gpu, tex, uv, g, mode, filt, 'box %d x %d ct=%d %s %s' % (box + (ct, mode, filt)))
            sizes.add((filt, box[0] * box[1]))
    assert {s for f, s in sizes if f == 'bilinear'} == {1600, 1640, 1602} and {s for f, s in sizes if f == 'nearest'} == {1600, 1640}


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 5])
def test_flat_list_patch_on_each_side_of_1600(gpu, ct):
    """A flat list of 256 look-ups (rows == 1: one 256 x 1 tile) walking a diagonal of the texture: a box of 40 x 40 = 1 600
    texels (the patch) and of 41 x 40 (atomics)."""
    rng = np.random.default_rng(60 + ct)
    tex = rng.uniform(-1, 1, (128, 128, ct)).astype(np.float32)
    g = rng.standard_normal((256, ct)).astype(np.float32)
    s = np.arange(256.) / 255
    for (dr, dc), box in (((38.25, 38.25), [40, 40]), ((39.0, 38.25), [41, 40])):
        uv = np.stack([(20.25 + dc * s) / 128, (20.25 + dr * s) / 128], -1).astype(np.float32)
        for mode in MODES:
            assert _tile_boxes(uv, 128, 128, mode, 'bilinear', 1, 256).tolist() == [[box]]
            _lookup(gpu, tex, uv, g, mode, 'bilinear', 'flat box %d x %d ct=%d %s' % (box[0], box[1], ct, mode))


# ---- the forward's grid-stride loop -----------------------------------------------------------------------------------

GRID_LANES = 16384 * 256   # capped_blocks: at most 16 384 workgroups of 256 lanes


@pytest.mark.gpu
@pytest.mark.parametrize('ct,filt,mode', [(1, 'bilinear', 'repeat'), (1, 'bilinear', 'clamp'), (1, 'nearest', 'repeat'), (1, 'nearest', 'clamp'),
                                          (3, 'nearest', 'repeat'), (3, 'nearest', 'clamp')])
def test_forward_past_the_grid_cap(gpu, ct, filt, mode):
    """4 194 304 + 300 flat look-ups: the last 300 are the second turn of the bilinear kernel's own grid-stride loop (and, for
    'nearest', of the `continue` in it).  The coordinates repeat a table of 4 099 pairs (a prime: no lane meets the same
    pair twice), so the oracle runs on the table; the whole output is compared bit for bit."""
    from dirt_amd import texture
    rng = np.random.default_rng(70)
    n, period = GRID_LANES + 300, 4099
    tex = rng.uniform(-1, 1, (13, 17, ct)).astype(np.float32)
    table = rng.uniform(-0.6, 1.6, (period, 2)).astype(np.float32)
    which = np.arange(n) % period
    out = texture.sample_texture_uv(_dev(gpu, tex), _dev(gpu, table[which]), mode, filt)
    assert out.shape == (n, ct)
    _forward_equal(out, tex_oracle.sample_texture_uv(tex, table, mode, filt)[which], 'past the grid cap ct=%d %s %s' % (ct, mode, filt))


# ---- write and read bounds, through ctypes ----------------------------------------------------------------------------

def _smooth_and_random(H, W, seed):
    """Two stacked images [2 * H, W, 2]: a smooth field with a `repeat` seam (patch tiles and, at the seam, atomic ones) and
    random coordinates (atomic tiles)."""
    rng = np.random.default_rng(seed)
    return np.concatenate([_smooth_uv(1, H, W, 1.1, seed)[0], rng.uniform(-0.5, 1.5, (H, W, 2)).astype(np.float32)])


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 5])
def test_guard_values_around_every_output(gpu, lib, ct):
    """Every operand inside a larger buffer: the inputs flush against the end of theirs (a 16-byte read of a 12-byte texel
    at the last texel of `texture` or the last pixel of `grad_out` would leave the tensor), the outputs between 64 floats
    of 123.0 on each side and pre-filled with it.  After the forward, the image backward and the flat backward: values
    as the oracle's, every guard float and -- with grad_uv_stride 5 and 7 -- every float between the pairs unchanged, and
    grad_texture, cleared by the call, exactly 0 in the texels no look-up touches."""
    Ht, Wt, H, W, n_flat = 19, 23, 37, 50, 1000
    rng = np.random.default_rng(80 + ct)
    tex = rng.uniform(-1, 1, (Ht, Wt, ct)).astype(np.float32)
    image = _smooth_and_random(H, W, ct)                                   # rows = 2 * H
    s = np.linspace(0, 1, n_flat // 2)
    flat = np.concatenate([np.stack([0.1 + 0.3 * s, 0.8 - 0.25 * s], -1), rng.uniform(-0.3, 0.6, (n_flat // 2, 2))]).astype(np.float32)
    t = _at_end(gpu, tex)
    for (mode, filt), guv_stride in ((('repeat', 'bilinear'), 5), (('clamp', 'bilinear'), 7), (('clamp', 'nearest'), 5), (('repeat', 'nearest'), 7)):
        c = _C(lib, gpu, tex.shape, mode, filt)
        for uv, rows, cols in ((image, 2 * H, W), (flat, 1, n_flat)):
            n = rows * cols
            what = 'ct=%d %s %s %d x %d' % (ct, mode, filt, rows, cols)
            g = rng.standard_normal((n, ct)).astype(np.float32)
            u, g_t = _at_end(gpu, uv), _at_end(gpu, g)
            obuf, out = _guarded(gpu, n * ct)
            c.forward(t, u, out, n)
            _forward_equal(out.view(uv.shape[:-1] + (ct,)), tex_oracle.sample_texture_uv(tex, uv, mode, filt), what + ' forward')
            assert _guards_intact(obuf, n * ct), what + ': the forward wrote outside `out`'
            tbuf, gtex = _guarded(gpu, tex.size)
            ubuf, guv = _guarded(gpu, n * guv_stride)
            if rows > 1:
                c.backward_image(t, u, g_t, gtex, guv, rows, cols, guv_stride=guv_stride)
            else:
                c.backward(t, u, g_t, gtex, guv, n, guv_stride=guv_stride)
            pairs = guv.view(n, guv_stride)
            _check_grads(gtex, pairs[:, :2], tex, uv, g, mode, filt, what)
            assert _guards_intact(tbuf, tex.size), what + ': the backward wrote outside grad_texture'
            assert _guards_intact(ubuf, n * guv_stride), what + ': the backward wrote outside grad_uvs'
            assert bool((pairs[:, 2:] == SENTINEL).all()), what + ': grad_uv_stride=%d wrote between the pairs' % guv_stride
            mass = tex_oracle.sample_texture_uv_grad(tex, uv, g, mode, filt, want_mass=True)[2]
            untouched = torch.from_numpy(mass == 0).to(gpu)
            assert rows > 1 or bool(untouched.any())                       # (the flat list leaves part of the texture alone)
            assert bool((gtex.view(tex.shape)[untouched] == 0).all()), what + ': grad_texture not cleared'


@pytest.mark.gpu
def test_the_clear_at_every_alignment_and_length(gpu, lib):
    """grad_texture is cleared by a kernel that stores float4 between the first and the last 16-byte boundary and single
    floats before and after: 1 to 9 floats (and 4 099) starting 0 to 3 floats past a boundary, pre-filled with the sentinel
    between guards; one look-up, so all but two floats are written by the clear alone."""
    uv, g = np.array([[0.3, 0.5]], np.float32), np.array([[2.0]], np.float32)
    u, g_t = _dev(gpu, uv), _dev(gpu, g)
    for wt in (1, 2, 3, 4, 5, 6, 7, 8, 9, 4099):
        tex = np.arange(1, wt + 1, dtype=np.float32).reshape(1, wt, 1)
        t = _dev(gpu, tex)
        c = _C(lib, gpu, tex.shape, 'clamp', 'bilinear')
        for off in range(4):
            buf = torch.full((GUARD + off + wt + GUARD,), SENTINEL, device=gpu)
            gtex = buf[GUARD + off:GUARD + off + wt]
            assert gtex.data_ptr() % 16 == 4 * off
            c.backward(t, u, g_t, gtex, None, 1)
            _check_grads(gtex, None, tex, uv, g, 'clamp', 'bilinear', '%d floats at %d mod 16' % (wt, 4 * off))
            assert bool((buf[:GUARD + off] == SENTINEL).all()) and bool((buf[GUARD + off + wt:] == SENTINEL).all()), (wt, off)


# ---- what the Python wrapper never passes -----------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 5])
def test_entry_points_with_what_python_never_passes(gpu, lib, ct):
    """NULL grad_uvs in both backward entry points; a forward uv_stride (6: channels 2:4 of a G-buffer) that differs from
    the backward's grad_uv_stride (3); the flat entry point on look-ups that form an image ("same results to summation
    order", include/dirt_hip.h); and one set of n look-ups given as 1 x n, n x 1 and H x W."""
    Ht, Wt, H, W = 21, 34, 24, 40
    n = H * W
    rng = np.random.default_rng(90 + ct)
    tex = rng.uniform(-1, 1, (Ht, Wt, ct)).astype(np.float32)
    gbuf = rng.uniform(-0.3, 1.3, (H, W, 6)).astype(np.float32)
    gbuf[..., 2:4] = _smooth_uv(1, H, W, 0.8, ct)[0]
    uv = np.ascontiguousarray(gbuf[..., 2:4])
    g = rng.standard_normal((H, W, ct)).astype(np.float32)
    t, gb, g_t = _dev(gpu, tex), _dev(gpu, gbuf), _dev(gpu, g)
    at_u = gb.data_ptr() + 4 * 2
    for mode in MODES:
        for filt in FILTERS:
            what = 'ct=%d %s %s' % (ct, mode, filt)
            c = _C(lib, gpu, tex.shape, mode, filt)
            out = torch.empty(H, W, ct, device=gpu)
            c.forward(t, at_u, out, n, uv_stride=6)
            _forward_equal(out, tex_oracle.sample_texture_uv(tex, uv, mode, filt), what + ' uv_stride=6 forward')
            for rows, cols in ((H, W), (1, n), (n, 1)):
                gtex, guv = torch.full_like(t, SENTINEL), torch.full((n, 3), SENTINEL, device=gpu)
                c.backward_image(t, at_u, g_t, gtex, guv, rows, cols, uv_stride=6, guv_stride=3)
                _check_grads(gtex, guv[:, :2], tex, uv, g, mode, filt, what + ' as %d x %d' % (rows, cols))
                assert bool((guv[:, 2] == SENTINEL).all())
                gtex2 = torch.full_like(t, SENTINEL)
                c.backward_image(t, at_u, g_t, gtex2, None, rows, cols, uv_stride=6, guv_stride=0)
                _check_grads(gtex2, None, tex, uv, g, mode, filt, what + ' as %d x %d, grad_uvs NULL' % (rows, cols))
            gtex, guv = torch.full_like(t, SENTINEL), torch.full((n, 3), SENTINEL, device=gpu)
            c.backward(t, at_u, g_t, gtex, guv, n, uv_stride=6, guv_stride=3)
            _check_grads(gtex, guv[:, :2], tex, uv, g, mode, filt, what + ' flat entry point on an image')
            assert bool((guv[:, 2] == SENTINEL).all())
            gtex2 = torch.full_like(t, SENTINEL)
            c.backward(t, at_u, g_t, gtex2, None, n, uv_stride=6)
            _check_grads(gtex2, None, tex, uv, g, mode, filt, what + ' flat entry point, grad_uvs NULL')


@pytest.mark.gpu
def test_tile_count_limit_is_refused_after_the_clear(gpu, lib):
    """cols = 2^31 does not fit the kernel's int: launch_texture_backward returns hipErrorInvalidValue (DIRT_E_HIP) after the
    call has cleared grad_texture, and does not launch the look-ups' kernel (grad_uvs keeps its sentinel)."""
    from dirt_amd import _lib, rasterise_ops as ops
    t, uv, g = torch.ones(1, device=gpu), torch.zeros(2, device=gpu), torch.ones(1, device=gpu)
    gtex, guv = torch.full((1,), SENTINEL, device=gpu), torch.full((2,), SENTINEL, device=gpu)
    rc = lib.dirt_texture_sample_backward_image(t.data_ptr(), uv.data_ptr(), g.data_ptr(), gtex.data_ptr(), guv.data_ptr(), 2, 1 << 31,
                                                1, 1, 1, 2, 2, 0, ops._stream_handle(gpu))
    assert rc == _lib.E_HIP and lib.dirt_texture_last_error() == (BWD + ': invalid argument').encode()
    torch.cuda.synchronize()
    assert gtex.item() == 0 and guv.tolist() == [SENTINEL, SENTINEL]
    rc = lib.dirt_texture_sample_backward(t.data_ptr(), uv.data_ptr(), g.data_ptr(), gtex.data_ptr(), None, 1 << 31, 1, 1, 1, 2, 2, 0,
                                          ops._stream_handle(gpu))
    assert rc == _lib.E_HIP and lib.dirt_texture_last_error() == (BWD + ': invalid argument').encode()
    torch.cuda.synchronize()


# ---- the pair-load test and the alignment dispatch --------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4])
@pytest.mark.parametrize('first,channels', [(0, 4), (2, 6), (4, 8), (1, 4), (3, 6)])
def test_uvs_in_place_from_even_stride_gbuffers(gpu, lib, ct, first, channels):
    """(u, v) read in place from channels first : first + 2 of a G-buffer with an even channel count: on an 8-byte boundary
    (0:2 of 4, 2:4 of 6, 4:6 of 8) the forward loads the pair in one access; at 4 mod 8 (1:3 of 4, 3:5 of 6) it loads
    scalars.  The coordinates' gradient is written in place into a G-buffer-shaped buffer (grad_uv_stride = channels) and
    must land in those two channels only."""
    H, W = 37, 50
    rng = np.random.default_rng(100 + 10 * first + ct)
    tex = rng.uniform(-1, 1, (26, 19, ct)).astype(np.float32)
    gbuf = rng.uniform(-0.3, 1.3, (2, H, W, channels)).astype(np.float32)
    gbuf[0, ..., first:first + 2] = _smooth_uv(1, H, W, 0.9, ct)[0]
    uv = np.ascontiguousarray(gbuf[..., first:first + 2])
    n = uv.size // 2
    g = rng.standard_normal((2, H, W, ct)).astype(np.float32)
    t, gb, g_t = _dev(gpu, tex), _dev(gpu, gbuf), _dev(gpu, g)
    assert gb.data_ptr() % 16 == 0
    at_u = gb.data_ptr() + 4 * first
    assert at_u % 8 == (0 if first % 2 == 0 else 4)
    for mode in MODES:
        for filt in FILTERS:
            what = 'channels %d:%d of %d ct=%d %s %s' % (first, first + 2, channels, ct, mode, filt)
            c = _C(lib, gpu, tex.shape, mode, filt)
            out = torch.empty(2, H, W, ct, device=gpu)
            c.forward(t, at_u, out, n, uv_stride=channels)
            _forward_equal(out, tex_oracle.sample_texture_uv(tex, uv, mode, filt), what + ' forward')
            gtex, ggb = torch.empty_like(t), torch.full_like(gb, SENTINEL)
            c.backward_image(t, at_u, g_t, gtex, ggb.data_ptr() + 4 * first, 2 * H, W, uv_stride=channels, guv_stride=channels)
            _check_grads(gtex, ggb[..., first:first + 2], tex, uv, g, mode, filt, what)
            assert bool((ggb[..., :first] == SENTINEL).all()) and bool((ggb[..., first + 2:] == SENTINEL).all()), what + ': wrote other channels'
    # ... and through the wrapper, which passes the slice in place
    from dirt_amd import texture
    gb.requires_grad_(True)
    out = texture.sample_texture_uv(t, gb[..., first:first + 2], 'repeat')
    _forward_equal(out, tex_oracle.sample_texture_uv(tex, uv, 'repeat'), 'wrapper forward')
    ggb, = torch.autograd.grad(out, [gb], g_t)
    want_uv, muv = tex_oracle.sample_texture_uv_grad(tex, uv, g, 'repeat', want_mass=True)[1::2]
    _per_element(ggb[..., first:first + 2], want_uv, muv, 'wrapper grad_uvs')
    assert not bool(ggb[..., :first].any()) and not bool(ggb[..., first + 2:].any())


@pytest.mark.gpu
@pytest.mark.parametrize('tex_off,io_off', [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_four_channels_in_every_alignment_combination(gpu, lib, tex_off, io_off):
    """Ct = 4: the forward takes its float4 kernel when `texture` AND `out` are 16-byte aligned, the backward when `grad_out`
    is, whatever `texture` is (it reads the texture scalar by scalar).  Each operand at 0 or 4 mod 16 bytes, asserted here:
    forward with texture aligned and out not, and the other way round; backward with grad_out aligned and texture not (the
    float4 kernel on a misaligned texture), and the other way round; and both corners."""
    Ht, Wt, H, W = 24, 40, 40, 48
    n = H * W
    rng = np.random.default_rng(110)
    tex = rng.uniform(-1, 1, (Ht, Wt, 4)).astype(np.float32)
    uv = _smooth_and_random(H // 2, W, 7)
    g = rng.standard_normal((H, W, 4)).astype(np.float32)
    t = _at_end(gpu, tex, lead=4 + tex_off)
    g_t = _at_end(gpu, g, lead=4 + io_off)
    obuf = torch.full((4 + io_off + n * 4 + 4,), SENTINEL, device=gpu)
    out = obuf[4 + io_off:4 + io_off + n * 4]
    u = _dev(gpu, uv)
    assert t.data_ptr() % 16 == 4 * tex_off and g_t.data_ptr() % 16 == 4 * io_off and out.data_ptr() % 16 == 4 * io_off
    for mode in MODES:
        for filt in FILTERS:
            what = 'texture at %d, out / grad_out at %d mod 16, %s %s' % (4 * tex_off, 4 * io_off, mode, filt)
            c = _C(lib, gpu, tex.shape, mode, filt)
            obuf.fill_(SENTINEL)
            c.forward(t, u, out, n)
            _forward_equal(out.view(H, W, 4), tex_oracle.sample_texture_uv(tex, uv, mode, filt), what + ' forward')
            assert bool((obuf[:4 + io_off] == SENTINEL).all()) and bool((obuf[4 + io_off + n * 4:] == SENTINEL).all())
            tbuf, gtex = _guarded(gpu, tex.size + 1)      # grad_texture takes the texture's alignment (the wrapper's empty_like would not)
            gtex = gtex[tex_off:tex_off + tex.size] if tex_off else gtex[:tex.size]
            guv = torch.empty(n, 2, device=gpu)
            c.backward_image(t, u, g_t, gtex, guv, H, W)
            _check_grads(gtex, guv, tex, uv, g, mode, filt, what)
            assert _guards_intact(tbuf, tex.size + 1) and tbuf[GUARD + (0 if tex_off else tex.size)].item() == SENTINEL


# ---- paths of the Python wrapper --------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('filt', FILTERS)
def test_empty_lookups(gpu, filt):
    from dirt_amd import texture
    t = torch.rand(5, 7, 3, device=gpu).requires_grad_(True)
    for shape in ((0, 2), (2, 0, 5, 2), (2, 3, 0, 2)):
        u = torch.zeros(shape, device=gpu).requires_grad_(True)
        out = texture.sample_texture_uv(t, u, 'repeat', filt)
        assert out.shape == shape[:-1] + (3,) and out.dtype == torch.float32
        gt, gu = torch.autograd.grad(out, [t, u], torch.zeros_like(out))
        assert gt.shape == t.shape and torch.equal(gt, torch.zeros_like(gt)), shape
        assert gu.shape == u.shape and gu.numel() == 0, shape


@pytest.mark.gpu
@pytest.mark.parametrize('filt', FILTERS)
def test_wrapper_conversions(gpu, filt):
    """What the wrapper converts before the call, with the gradient coming back through the conversion: a float64 texture and
    float64 coordinates (float64 gradients with the float32 run's values), a non-contiguous texture, coordinates expanded
    over a batch (their gradient sums over the expansion) and transposed."""
    from dirt_amd import texture
    Ht, Wt, H, W, ct = 17, 22, 20, 36, 3
    rng = np.random.default_rng(120)
    tex = rng.uniform(-1, 1, (Ht, Wt, ct)).astype(np.float32)
    uv = _smooth_uv(1, H, W, 1.2, 5)[0]
    g = rng.standard_normal((H, W, ct)).astype(np.float32)
    for mode in MODES:
        want = tex_oracle.sample_texture_uv(tex, uv, mode, filt)
        # float64 in, float64 gradients out
        t, u = _dev(gpu, tex).double().requires_grad_(True), _dev(gpu, uv).double().requires_grad_(True)
        out = texture.sample_texture_uv(t, u, mode, filt)
        assert out.dtype == torch.float32
        _forward_equal(out, want, 'float64 %s forward' % mode)
        gt, gu = torch.autograd.grad(out, [t, u], _dev(gpu, g))
        assert gt.dtype == torch.float64 and gu.dtype == torch.float64
        _check_grads(gt, gu, tex, uv, g, mode, filt, 'float64 %s' % mode)
        # a non-contiguous texture: the [Wt, Ht, C] buffer seen as [Ht, Wt, C]
        held = _dev(gpu, tex.transpose(1, 0, 2)).requires_grad_(True)
        t = held.permute(1, 0, 2)
        assert not t.is_contiguous()
        u = _dev(gpu, uv).requires_grad_(True)
        out = texture.sample_texture_uv(t, u, mode, filt)
        _forward_equal(out, want, 'permuted texture %s forward' % mode)
        gt, gu = torch.autograd.grad(out, [held, u], _dev(gpu, g))
        _check_grads(gt.permute(1, 0, 2), gu, tex, uv, g, mode, filt, 'permuted texture %s' % mode)
        # transposed coordinates: a [W, H, 2] leaf seen as [H, W, 2]
        t = _dev(gpu, tex).requires_grad_(True)
        held = _dev(gpu, uv.transpose(1, 0, 2)).requires_grad_(True)
        out = texture.sample_texture_uv(t, held.transpose(0, 1), mode, filt)
        _forward_equal(out, want, 'transposed uvs %s forward' % mode)
        gt, gu = torch.autograd.grad(out, [t, held], _dev(gpu, g))
        _check_grads(gt, gu.transpose(0, 1), tex, uv, g, mode, filt, 'transposed uvs %s' % mode)
        # expanded coordinates: three views of one [H, W, 2] leaf
        g3 = rng.standard_normal((3, H, W, ct)).astype(np.float32)
        uv3 = np.broadcast_to(uv, (3,) + uv.shape)
        u = _dev(gpu, uv).requires_grad_(True)
        out = texture.sample_texture_uv(t, u[None].expand(3, H, W, 2), mode, filt)
        _forward_equal(out, tex_oracle.sample_texture_uv(tex, uv3, mode, filt), 'expanded uvs %s forward' % mode)
        gt, gu = torch.autograd.grad(out, [t, u], _dev(gpu, g3))
        want_t, want_uv, mt, muv = tex_oracle.sample_texture_uv_grad(tex, uv3, g3, mode, filt, want_mass=True)
        _per_element(gt, want_t, mt, 'expanded uvs %s grad_texture' % mode)
        _per_element(gu, want_uv.astype(np.float64).sum(0), muv.sum(0), 'expanded uvs %s grad_uvs' % mode)


@pytest.mark.gpu
def test_on_a_side_stream(gpu):
    """The look-up, the clear of grad_texture and the backward kernel all go to the current stream, not the default one."""
    from dirt_amd import texture
    rng = np.random.default_rng(130)
    tex = rng.uniform(-1, 1, (40, 30, 4)).astype(np.float32)
    uv = _smooth_and_random(48, 64, 3)
    g = rng.standard_normal(uv.shape[:-1] + (4,)).astype(np.float32)
    t, u, g_t = _dev(gpu, tex).requires_grad_(True), _dev(gpu, uv).requires_grad_(True), _dev(gpu, g)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        out = texture.sample_texture_uv(t, u, 'repeat')
        gt, gu = torch.autograd.grad(out, [t, u], g_t)
    side.synchronize()
    _forward_equal(out, tex_oracle.sample_texture_uv(tex, uv, 'repeat'), 'side stream forward')
    _check_grads(gt, gu, tex, uv, g, 'repeat', 'bilinear', 'side stream')
    torch.cuda.current_stream(gpu).wait_stream(side)


@pytest.mark.gpu
@pytest.mark.parametrize('filt', FILTERS + ('trilinear',))
def test_a_captured_lookup_and_backward_replay_on_new_textures(gpu, filt):
    """The look-up and its backward (the clear of grad_texture and a kernel) make no host synchronisation: captured with
    torch.cuda.graph and replayed three times, the texture rewritten in place before each replay; every replay's look-up
    equals the oracle's for that texture bit for bit and its gradients are within tolerance (float atomics: not to the bit).
    The clear is the point: part of the texture is touched by no look-up and must come back 0 on EVERY replay -- as a
    captured hipMemsetAsync it did on the first replay only.  'trilinear' (dirt_texture_mip.hip clears its pyramid-shaped
    scratch the same way) against tests/mip_reference.py at that file's tolerance."""
    from dirt_amd import texture
    from tests import mip_reference as mr
    from tests.test_texture_mip_edges import _close
    rng = np.random.default_rng(140)
    Ht, Wt, ct = 32, 28, 3
    tex = rng.uniform(-1, 1, (Ht, Wt, ct)).astype(np.float32)
    uv = np.concatenate([_smooth_uv(1, 24, 40, 0.5, 4, seam=False)[0], rng.uniform(0.1, 0.65, (24, 40, 2)).astype(np.float32)])   # u, v < 0.7
    lod = rng.uniform(-0.5, 2.5, uv.shape[:-1]).astype(np.float32)
    g = rng.standard_normal(uv.shape[:-1] + (ct,)).astype(np.float32)
    t, u, g_t = _dev(gpu, tex), _dev(gpu, uv), _dev(gpu, g)
    kw = {'lod': _dev(gpu, lod)} if filt == 'trilinear' else {}
    assert (tex_oracle.sample_texture_uv_grad(tex, uv, g, 'repeat', 'bilinear', want_mass=True)[2] == 0).sum() >= 10 * ct   # texels only the clear writes

    def step():
        leaves = [x.detach().requires_grad_(True) for x in (t, u)]
        out = texture.sample_texture_uv(leaves[0], leaves[1], 'repeat', filt, **kw)
        return (out.detach(),) + tuple(torch.autograd.grad(out, leaves, g_t))

    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g, gt_g, gu_g = step()
    for k in range(3):
        tex_k = rng.uniform(-1, 1, tex.shape).astype(np.float32)
        with torch.no_grad():
            t.copy_(_dev(gpu, tex_k))
        graph.replay()
        torch.cuda.synchronize()
        if filt == 'trilinear':
            want, mag = mr.sample(tex_k, uv, 'repeat', lod=lod, magnitude=True)
            _close(out_g, want, mag, 'replay %d forward' % k)
            r = mr.grad(tex_k, uv, g, 'repeat', lod=lod)
            _close(gt_g, r['grad_texture'], r['mass_texture'], 'replay %d grad_texture' % k)
            _close(gu_g, r['grad_uvs'], r['mass_uvs'], 'replay %d grad_uvs' % k)
            assert (r['mass_texture'] == 0).sum() >= 10 * ct and bool((gt_g[torch.from_numpy(r['mass_texture'] == 0).to(gpu)] == 0).all())
        else:
            _forward_equal(out_g, tex_oracle.sample_texture_uv(tex_k, uv, 'repeat', filt), 'replay %d forward' % k)
            _check_grads(gt_g, gu_g, tex_k, uv, g, 'repeat', filt, 'replay %d' % k)


# ---- denormals and extremes -------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 5])
def test_extreme_and_denormal_coordinates(gpu, ct):
    """Coordinates +-1e-40 (float32 denormals), +-1e30, +-(2^24 + 1), +-FLT_MAX in u and v, crossed with each other and with
    ordinary values, in both modes and filters.  -1e-40 in 'repeat' is the telling one: -1e-40 - floor(-1e-40) rounds to 1,
    the last texel; flushed to -0 it would read texel 0.  Every special column / row also holds look-ups at ordinary
    coordinates, so each texel's mass has terms of ordinary size (the tolerance is relative to the mass; a denormal weight
    alone has a float32 rounding error of up to 2^-150, about 1e-5 of 1e-40)."""
    rng = np.random.default_rng(150 + ct)
    Ht, Wt = 6, 9
    tex = rng.uniform(0.5, 1.5, (Ht, Wt, ct)).astype(np.float32)
    fmax = float(np.finfo(np.float32).max)
    vals = np.array([1e-40, -1e-40, 1e30, -1e30, 2.0 ** 24 + 1, -(2.0 ** 24 + 1), fmax, -fmax, 0.0, 1.0, 0.3, 0.77], np.float64).astype(np.float32)
    us = np.concatenate([vals, (np.array([0.5, Wt - 0.5, 0.25]) / Wt).astype(np.float32)])
    vs = np.concatenate([vals, (np.array([0.5, Ht - 0.5, 0.25]) / Ht).astype(np.float32)])
    uv = np.stack(np.meshgrid(us, vs), -1).astype(np.float32)
    g = (rng.uniform(0.5, 1.5, uv.shape[:-1] + (ct,)) * rng.choice([-1.0, 1.0], uv.shape[:-1] + (ct,))).astype(np.float32)
    assert tex_oracle.sample_texture_uv(tex, np.array([[-1e-40, 0.0]], np.float32), 'repeat', 'nearest')[0, 0] == tex[0, Wt - 1, 0]
    for mode in MODES:
        for filt in FILTERS:
            _lookup(gpu, tex, uv, g, mode, filt, 'extreme coordinates ct=%d %s %s' % (ct, mode, filt))
            _lookup(gpu, tex, uv.reshape(-1, 2), g.reshape(-1, ct), mode, filt, 'extreme coordinates, flat, ct=%d %s %s' % (ct, mode, filt))


def _exact_case(ct, shift, spread, offset, seed):
    """A look-up whose every float32 operation is EXACT when denormals are kept, so that the kernels' float32 results equal
    the float64 oracle's: a 64 x 64 texture (a power of two: the index is the coordinate scaled exactly), coordinates on
    multiples of 1 / 128 (fractions 0 or 0.5: weights 0, 0.25, 0.5, 1), texels and grad_out small integers times a power
    of two per channel kind --
      kind 0: texels k, grad_out k * 2^-136 (denormal): grad_texture sums denormals; the terms of grad_uvs are denormal;
      kind 1: texels k * 2^-136 (denormal), grad_out k: the look-up blends denormals;
      kind 2: texels k * 2^-70, grad_out k * 2^-70: the products of grad_uvs underflow into the denormals, exactly;
    channel j is of kind (j + shift) % 3.  One look-up in eight has grad_out k * 2^-100 in its channels of kind 2: those
    products (2^-170 k) underflow to zero in float32 and change no float32 rounding of the float64 sums they enter."""
    rng = np.random.default_rng(seed)
    kinds = (np.arange(ct) + shift) % 3
    t_scale = np.array([1.0, 2.0 ** -136, 2.0 ** -70])[kinds]
    g_scale = np.array([2.0 ** -136, 1.0, 2.0 ** -70])[kinds]
    tex = (rng.integers(1, 9, (64, 64, ct)) * t_scale).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(16), np.arange(16), indexing='ij')
    uv = np.stack([(xs * spread + 0.5 * (xs % 2) + offset) / 64, (ys * spread + 0.5 * ((ys + 1) % 2) + offset) / 64], -1).astype(np.float32)
    g = rng.integers(1, 8, (16, 16, ct)) * rng.choice([-1, 1], (16, 16, ct)) * g_scale
    small = rng.uniform(0, 1, (16, 16)) < 0.125
    g[small] = g[small] / g_scale * np.where(kinds == 2, 2.0 ** -100, g_scale)
    return tex, uv, g.astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize('ct', [1, 3, 4, 5])
def test_denormal_texels_and_gradients(gpu, ct):
    """Denormal texels, denormal grad_out and products that underflow, on inputs for which float32 arithmetic that keeps
    denormals is exact (_exact_case): the look-up bit for bit, the gradients within tolerance of the mass -- which a value
    flushed to zero is not.  One tile that takes the LDS patch (a 17 x 17 box) and one that takes global atomics (a seam in
    'repeat', a 45 x 45 box in 'clamp'), both modes and filters, every kind of channel in every kernel."""
    for shift in range(3):
        for spread, offset, patch in ((1, 2, True), (3, -2, False)):
            tex, uv, g = _exact_case(ct, shift, spread, offset, 160 + 3 * ct + shift)
            for mode in MODES:
                for filt in FILTERS:
                    bh, bw = _tile_boxes(uv, 64, 64, mode, filt, 16, 16)[0, 0]
                    assert (bh * bw <= TEX_PATCH) == patch, (mode, filt, bh, bw)
                    _lookup(gpu, tex, uv, g, mode, filt, 'denormals ct=%d shift=%d %s %s %s' % (ct, shift, 'patch' if patch else 'atomics', mode, filt))
