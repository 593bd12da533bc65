"""The four-pixels-per-lane gradient kernel where its memory trips were moved (dirt_grad.hip: every load of a wave in one burst,
the state tile's stores unconditional with clamped duplicates): frames smaller than a tile and not multiples of one, with
partial waves and clamped rows and columns, a scene built so that both ring cells of a lane receive something, the
aliased-inbox form as the library itself picks it, and non-finite values at a ring cell.  Against the CPU oracle:
grad_background bit for bit, vertex gradients within parity.TIGHT_TOL of each element's own terms (tests/parity.py).
(Pixel tensors that are not 16-byte aligned cannot reach the kernels: the C ABI rejects them and the wrapper copies such views;
test_ring_scene_with_misaligned_views checks that copy on the ring scene.)"""
import numpy as np
import pytest
import torch

from dirt_amd import rasterise_ops as ops
from tests import parity, scenes
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu

PX4, PAIRS, ROWS = 0x10000, 0x2000, 0x1000   # DIRT_FLAG_GRAD_PX4 / _PAIRS / _ROWS
SHAPES = [pytest.param(PX4 | PAIRS, id='pairs'), pytest.param(PX4 | ROWS, id='rows')]


def _check(gpu, oracle, b, H, W, C, flags, what, want=None, ow=None):
    """Forward on the GPU (bit-exact), then the backward with and without the forward's state, against the oracle."""
    if want is None:
        want = oracle.forward(b['background'], b['vertices'], b['vertex_colors'], b['faces'])
    if ow is None:
        ow = oracle.backward(b['vertices'], b['faces'], want, b['grad_pixels'])
    d = {k: _t(b[k], gpu) for k in ('background', 'vertices', 'vertex_colors', 'faces', 'grad_pixels')}
    px, state = ops._op_rasterise(d['background'], d['vertices'], d['vertex_colors'], d['faces'], H, W, C, keep_state=True)
    assert np.array_equal(px.cpu().numpy().view(np.uint32), want.view(np.uint32)), what + ': pixels'
    for st in (state, None):
        gb, gv, gvc, _ = ops._op_rasterise_grad(d['vertices'], d['faces'], px, d['grad_pixels'], H, W, C, flags=flags, state=st)
        assert np.array_equal(gb.cpu().numpy().view(np.uint32), ow['grad_background'].view(np.uint32)), what + ': grad_background'
        parity.grads_close(gv, gvc, ow, what, tol=parity.TIGHT_TOL)


# ---- frames smaller than, or not a multiple of, a tile: partial waves, ring cells and prefetch addresses outside the frame ----
_small_cache = {}


def _small(oracle, H, W, C):
    key = (H, W, C)
    if key not in _small_cache:
        s = scenes.rand_scene(8, H, W, C, 7 + H + 3 * W, 0.4, 1.2)   # a handful of large triangles that overlap in depth
        b = {k: s[k][None] for k in ('background', 'vertices', 'vertex_colors', 'faces', 'grad_pixels')}
        want = oracle.forward(b['background'], b['vertices'], b['vertex_colors'], b['faces'])
        _small_cache[key] = (b, want, oracle.backward(b['vertices'], b['faces'], want, b['grad_pixels']))
    return _small_cache[key]


@pytest.mark.parametrize('C', [4, 1, 3])
@pytest.mark.parametrize('H,W', [(1, 1), (5, 3), (33, 9), (40, 32), (65, 31), (3, 5), (9, 33), (31, 65)])
@pytest.mark.parametrize('flags', SHAPES)
def test_small_and_partial_frames(gpu, oracle, H, W, C, flags):
    b, want, ow = _small(oracle, H, W, C)
    _check(gpu, oracle, b, H, W, C, flags, '%dx%dx%d' % (H, W, C), want, ow)


# ---- a 64 x 64 scene built for the ring: near quads over a far one, their edges on the tile border x = 32 and on the wave and
#      tile borders y = 8, 16, 24, 32, one corner on (32, 32) ----
def _quad(x0, x1, y0, y1, z, w, H=64, W=64):
    """Two triangles over the pixel rectangle [x0, x1) x [y0, y1) (tensor rows, top row first) at constant clip_w."""
    def v(x, y):
        return [(2.0 * x / W - 1.0) * w, (1.0 - 2.0 * y / H) * w, z * w, w]
    return [v(x0, y0), v(x1, y0), v(x1, y1), v(x0, y1)]


RING_QUADS = [(0, 64, 0, 60, 0.5, 3.0),      # far: the whole frame but its last four rows (background there)
              (32, 56, 8, 16, 0.00, 1.5),    # near, right of x = 32, between y = 8 and y = 16
              (8, 32, 16, 24, -0.05, 1.7),   # left of x = 32, y = 16 .. 24
              (32, 60, 24, 32, -0.10, 1.9),  # right again, y = 24 .. 32: its lower left corner is (32, 32)
              (4, 32, 32, 44, -0.15, 2.1),   # below the tile border y = 32, upper right corner on (32, 32)
              (8, 24, 2, 8, -0.20, 2.3)]     # above y = 8 on the left: what wave 1's top ring cells receive


def _ring_scene(C, seed=3, quads=RING_QUADS):
    H = W = 64
    verts, faces = [], []
    for q in quads:
        n = len(verts)
        verts += _quad(*q)
        faces += [[n, n + 1, n + 2], [n, n + 2, n + 3]]
    rng = np.random.default_rng(seed)
    V = len(verts)
    return dict(background=rng.uniform(0, 1, [1, H, W, C]).astype(np.float32), vertices=np.asarray(verts, np.float32)[None],
                faces=np.asarray(faces, np.int32)[None], vertex_colors=rng.uniform(0, 1, [1, V, C]).astype(np.float32),
                grad_pixels=rng.standard_normal([1, H, W, C]).astype(np.float32))


_ring_cache = {}


def _ring(oracle, C):
    if C not in _ring_cache:
        b = _ring_scene(C)
        want = oracle.forward(b['background'], b['vertices'], b['vertex_colors'], b['faces'])
        ow = oracle.backward(b['vertices'], b['faces'], want, b['grad_pixels'], want_debug=True)
        _ring_cache[C] = (b, want, ow)
    return _ring_cache[C]


def _assert_ring_is_exercised(ow):
    """From the oracle's debug output: far pixels next to the near quads' edges are dilated across each of the five lines, on
    both sides of x = 32; and wave 1 of the first tile (rows 8 .. 15) gets something into its top ring cells 12 .. 19 (row 7 from
    row 8) AND into its right column (column 32 from column 31): ring cells 0 and 1 of lanes 12 .. 19."""
    D = ow['debug_thingy'][0, :, :, 0] != 0
    for name, region in (('y=8', D[7, 33:55]), ('y=16 from below', D[16, 33:55]), ('y=16 from above', D[15, 9:31]),
                         ('y=24 from below', D[24, 9:31]), ('y=24 from above', D[23, 33:59]), ('y=32 from below', D[32, 33:59]),
                         ('y=32 from above', D[31, 5:31]), ('x=32 from the left', D[9:15, 31]), ('x=32 from the right', D[17:23, 32]),
                         ('row 8 upwards, cells 12..19', D[8, 11:19])):
        assert region.any(), 'the scene does not dilate across ' + name


@pytest.mark.parametrize('C', [4, 1, 3])
@pytest.mark.parametrize('flags', SHAPES)
def test_ring_scene(gpu, oracle, C, flags):
    b, want, ow = _ring(oracle, C)
    _assert_ring_is_exercised(ow)
    _check(gpu, oracle, b, 64, 64, C, flags, 'ring scene C=%d' % C, want, ow)


@pytest.mark.parametrize('flags', SHAPES)
def test_ring_scene_with_misaligned_views(gpu, oracle, flags):
    """`pixels` and `grad_pixels` as views that start one float into their buffers (the C ABI takes 16-byte aligned tensors: the
    wrapper copies such views, as test_misaligned_views_are_accepted has it), the results as the aligned call's."""
    b, want, ow = _ring(oracle, 4)
    n = want.size
    pbuf, gbuf = torch.zeros(n + 1, device=gpu), torch.zeros(n + 1, device=gpu)
    pbuf[1:] = _t(want.reshape(-1), gpu)
    gbuf[1:] = _t(b['grad_pixels'].reshape(-1), gpu)
    px, gp = pbuf[1:].view(1, 64, 64, 4), gbuf[1:].view(1, 64, 64, 4)
    assert px.data_ptr() % 16 != 0 and gp.data_ptr() % 16 != 0
    gb, gv, gvc, _ = ops._op_rasterise_grad(_t(b['vertices'], gpu), _t(b['faces'], gpu), px, gp, 64, 64, 4, flags=flags)
    assert np.array_equal(gb.cpu().numpy().view(np.uint32), ow['grad_background'].view(np.uint32))
    parity.grads_close(gv, gvc, ow, 'misaligned views', tol=parity.TIGHT_TOL)


def test_aliased_inbox_form(gpu, oracle):
    """One launch of 2 048 frames of 9 x 7 with four faces each: 2 048 workgroups, from which on the library takes the form whose
    inbox is aliased onto the pixel planes (pick_grad_shape).  Every frame against the oracle."""
    B, H, W, C = 2048, 7, 9, 4
    b = scenes.batch_scene(4, H, W, C, seeds=list(range(500, 500 + B)), r_lo=0.4, r_hi=1.2)
    _check(gpu, oracle, b, H, W, C, 0, '2048 frames of 9x7')


@pytest.mark.parametrize('flags', SHAPES)
def test_non_finite_values_at_a_ring_cell(gpu, oracle, flags):
    """A NaN and an Inf in grad_pixels at pixels whose dilation target is a ring cell of their wave (row 7 into row 8, column 31
    into column 32), and a near quad whose clip_w is so small that every position term of its vertices overflows: what
    test_non_finite_grad_pixels_stay_with_their_own_face expects -- non-finite exactly where the oracle's gradients are,
    within the tolerance elsewhere, grad_background bit for bit (the NaN of an uncovered pixel included)."""
    quads = list(RING_QUADS)
    quads[5] = (8, 24, 2, 8, -0.20, 1e-37)   # the quad above y = 8: 32 / clip_w is not finite
    b = _ring_scene(4, quads=quads)
    want = oracle.forward(b['background'], b['vertices'], b['vertex_colors'], b['faces'])
    D = oracle.backward(b['vertices'], b['faces'], want, b['grad_pixels'], want_debug=True)['debug_thingy'][0, :, :, 0] != 0
    g = b['grad_pixels']
    g[0, 0:10, 6:26, :] *= 1e4               # over and around that quad: every term its vertices receive overflows, in any order of summation
    xs7, ys31, xs8 = np.flatnonzero(D[7, 33:55]) + 33, np.flatnonzero(D[9:15, 31]) + 9, np.flatnonzero(D[8, 9:23]) + 9
    assert xs7.size >= 2 and ys31.size >= 1 and xs8.size >= 1, 'the scene does not dilate into the ring'
    g[0, 7, xs7[0], 1] = np.nan
    g[0, 7, xs7[1], 2] = np.inf
    g[0, ys31[0], 31, 0] = -np.inf
    g[0, 62, 5, 3] = np.nan                  # an uncovered pixel: grad_background carries it
    ow = oracle.backward(b['vertices'], b['faces'], want, g)
    assert not np.isfinite(ow['grad_vertices']).all() and np.isfinite(ow['grad_vertices']).any()
    assert not np.isfinite(ow['grad_vertices'][0, 20:24][:, [0, 1, 3]]).any(), 'a position gradient of the degenerate quad is finite'
    d = {k: _t(b[k], gpu) for k in b}
    px, state = ops._op_rasterise(d['background'], d['vertices'], d['vertex_colors'], d['faces'], 64, 64, 4, keep_state=True)
    for st in (state, None):
        gb, gv, gvc, _ = ops._op_rasterise_grad(d['vertices'], d['faces'], px, d['grad_pixels'], 64, 64, 4, flags=flags, state=st)
        assert np.array_equal(gb.cpu().numpy().view(np.uint32), ow['grad_background'].view(np.uint32)), 'grad_background'
        parity.grads_close(gv, gvc, ow, 'non-finite values at a ring cell')
