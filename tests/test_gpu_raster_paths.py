"""The paths of raster_kernel_v2 (dirt_forward.hip) that its prologue and its shading pass branch on and that no other test
names, each against the CPU oracle (never the library against itself).  The colour mode runs in both shapes of the kernel --
four waves of 16 x 16 pixels, eight waves of 16 x 8 (DIRT_FLAG_TILES_LARGE, | DIRT_FLAG_TILES_SMALL) --; the visibility mode
has the four-wave shape only (both parametrisations run that one kernel), as has the stateless backward pass's export:

  * a frame whose every wave region is pure background (an empty mesh: no thread holds a directory cell; a mesh whose every
    face is culled);
  * a frame in which the pixels a lane holds (8 apart in x, and in y in the four-wave shape) never have the same winner;
  * meshes of 1, 64, 65 and 256 chunks of 64 faces, a chunk's cell per thread: one, one, two and four waves hold cells, which
    is one, one, two and four of the eight waves and one, one, two and all of the four;
  * tiles with more than 96 candidates: later rounds, winners whose shading data comes from memory;
  * frame sizes not divisible by 32 in either direction (every frame here);
  * one workspace used for a dense scene, a sparse one and the dense one again: stale LDS / list state would show.

Inputs are generated from seeds.  What a case needs of its input (covered and uncovered pixels, differing winners, candidates
per tile) is asserted on the oracle's output before the library is looked at."""
import ctypes

import numpy as np
import pytest
import torch

from dirt_amd import _lib, rasterise_ops as ops
from tests import parity, scenes

pytestmark = pytest.mark.gpu

# the forward kernel's shape, with one of the gradient kernel's face-loop shapes pinned as tests/test_gpu_parity.py does
SHAPES = [pytest.param(0x200 | 0x2000, id='four-waves'), pytest.param(0x600 | 0x2000, id='eight-waves')]
V2_CAP = 96   # candidates per round of raster_kernel_v2 (DIRT_V2_CAP)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _scene(verts, faces, H, W, C, seed):
    rng = np.random.default_rng(seed)
    return dict(background=rng.uniform(0, 1, [H, W, C]).astype(np.float32), vertices=np.asarray(verts, np.float32),
                faces=np.asarray(faces, np.int32).reshape(-1, 3), vertex_colors=rng.uniform(0, 1, [len(verts), C]).astype(np.float32),
                grad_pixels=rng.standard_normal([H, W, C]).astype(np.float32), height=H, width=W, channels=C)


def checker_scene(H, W, C, seed, cell=4):
    """Every other cell of a grid of cell x cell pixels holds a quad of two small triangles of its own (split vertices, a depth
    and a w of its own): pixels 8 apart, in x or in y, never share a face; the other cells stay background."""
    rng = np.random.default_rng(seed)
    verts, faces = [], []
    for cy in range((H + cell - 1) // cell):
        for cx in range((W + cell - 1) // cell):
            if (cx + cy) & 1:
                continue
            x0, x1 = 2.0 * cx * cell / W - 1.0, 2.0 * (cx + 1) * cell / W - 1.0
            y0, y1 = 2.0 * cy * cell / H - 1.0, 2.0 * (cy + 1) * cell / H - 1.0
            z = rng.uniform(-0.9, 0.9)
            for tri in (((x0, y0), (x1, y0), (x1, y1)), ((x0, y0), (x1, y1), (x0, y1))):
                base = len(verts)
                for (x, y) in tri:
                    w = rng.uniform(1, 4)
                    verts.append([x * w, y * w, z * w, w])
                faces.append([base, base + 1, base + 2])
    return _scene(verts, faces, H, W, C, seed + 1)


def culled_scene(H, W, C, seed, F=200):
    """Random triangles, every one of them behind the eye (w < 0 at all three vertices): set-up drops them all."""
    v, f = scenes.rand_mesh(F, seed, 0.05, 0.3)
    return _scene(-v, f, H, W, C, seed + 1)


def empty_scene(H, W, C, seed):
    return _scene(np.zeros([0, 4], np.float32), np.zeros([0, 3], np.int32), H, W, C, seed)


def _candidates_per_tile(s):
    """Lower bound of the candidates of the busiest 32 x 32 tile: faces whose pixel box (all w > 0 here) touches it."""
    H, W = s['height'], s['width']
    v = s['vertices'][s['faces']]                                  # [F, 3, 4]
    x = (v[..., 0] / v[..., 3] + 1.0) * 0.5 * W
    y = (1.0 - (v[..., 1] / v[..., 3] + 1.0) * 0.5) * H             # rows from the top
    best = 0
    for ty in range((H + 31) // 32):
        for tx in range((W + 31) // 32):
            inside = (x.max(1) >= 32 * tx + 1) & (x.min(1) <= 32 * tx + 31) & (y.max(1) >= 32 * ty + 1) & (y.min(1) <= 32 * ty + 31)
            best = max(best, int(inside.sum()))
    return best


def oracle_side(oracle, s):
    """(pixels, face ids) of the oracle for one scene; the oracle accepting the input is part of the check."""
    want = oracle.forward(s['background'][None], s['vertices'][None], s['vertex_colors'][None], s['faces'][None])
    vis, _, _ = oracle.visibility(s['vertices'], s['faces'], s['height'], s['width'])
    assert want.shape == (1, s['height'], s['width'], s['channels']) and np.all(np.isfinite(want))
    return want, vis


def _visibility_gpu(s, dev, flags):
    """dirt_rasterise_visibility with the tile shape pinned (the op of dirt_amd.rasterise_ops takes no flags)."""
    lib = _lib.load()
    v, f = _t(s['vertices'][None], dev), _t(s['faces'][None], dev)
    H, W = s['height'], s['width']
    out = torch.empty((1, H, W), dtype=torch.int32, device=dev)
    n = lib.dirt_workspace_bytes(1, v.shape[1], f.shape[1], H, W, 1)
    ws = torch.empty(max(int(n), 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.dirt_rasterise_visibility(v.data_ptr(), f.data_ptr(), out.data_ptr(), 1, v.shape[1], f.shape[1], H, W,
                                                 ws.data_ptr(), ws.numel(), flags & 0x600, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    torch.cuda.synchronize(dev)
    return out[0].cpu().numpy()


def _forward_gpu(s, dev, flags, keep_state=False):
    return ops._op_rasterise(_t(s['background'][None], dev), _t(s['vertices'][None], dev), _t(s['vertex_colors'][None], dev),
                             _t(s['faces'][None], dev), s['height'], s['width'], s['channels'], flags=flags & 0x600, keep_state=keep_state)


def check_against_oracle(s, want, vis, oracle, dev, shape, what, gradients=True):
    """Pixels and face ids bit for bit; then the two state planes through what reads them: the backward pass from the kept
    state (colour mode's export) and the stateless one (visibility mode's export), grad_background bit for bit and the vertex
    gradients at tests/parity.py's tolerance."""
    px, state = _forward_gpu(s, dev, shape, keep_state=True)
    got = px.cpu().numpy()
    nbad = int(np.sum(got.view(np.uint32) != want.view(np.uint32)))
    assert nbad == 0, '%s: %d of %d pixel values differ from the oracle' % (what, nbad, got.size)
    gvis = _visibility_gpu(s, dev, shape)
    assert np.array_equal(gvis, vis), '%s: %d face ids differ from the oracle' % (what, int(np.sum(gvis != vis)))
    if not gradients or s['vertices'].shape[0] == 0:
        return
    H, W, C = s['height'], s['width'], s['channels']
    ow = oracle.backward(s['vertices'][None], s['faces'][None], want, s['grad_pixels'][None])
    args = (_t(s['vertices'][None], dev), _t(s['faces'][None], dev), _t(want, dev), _t(s['grad_pixels'][None], dev), H, W, C)
    for label, kw in (('kept state', dict(state=state, state_outputs=False)), ('stateless', dict())):
        gb, gv, gvc, _ = ops._op_rasterise_grad(*args, flags=shape, **kw)
        assert np.array_equal(gb.cpu().numpy(), ow['grad_background']), '%s (%s): grad_background' % (what, label)
        parity.grads_close(gv, gvc, ow, '%s (%s)' % (what, label), index=None, tol=parity.TIGHT_TOL)


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('C', [1, 3, 4])
@pytest.mark.parametrize('kind', ['empty', 'culled'])
def test_every_wave_region_is_background(gpu, oracle, shape, C, kind):
    s = empty_scene(70, 90, C, 31) if kind == 'empty' else culled_scene(70, 90, C, 32)
    if kind == 'empty':   # (the oracle's visibility of no faces: nothing to ask it)
        want, vis = s['background'][None].copy(), np.full((70, 90), -1, np.int32)
    else:
        want, vis = oracle_side(oracle, s)
    assert np.all(vis == -1) and np.array_equal(want[0], s['background']), 'the case wants no covered pixel'
    check_against_oracle(s, want, vis, oracle, gpu, shape, kind + ' C=%d' % C, gradients=kind != 'empty')


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('H,W,C', [(70, 90, 4), (45, 107, 3), (95, 33, 1)])
def test_a_lanes_pixels_never_share_a_winner(gpu, oracle, shape, H, W, C):
    s = checker_scene(H, W, C, 41)
    want, vis = oracle_side(oracle, s)
    assert np.any(vis >= 0) and np.any(vis < 0), 'the case wants covered and uncovered pixels'
    a, b = vis[:, :-8], vis[:, 8:]
    assert not np.any((a >= 0) & (a == b)), 'pixels 8 apart in x share a winner'
    a, b = vis[:-8, :], vis[8:, :]
    assert not np.any((a >= 0) & (a == b)), 'pixels 8 apart in y share a winner'
    check_against_oracle(s, want, vis, oracle, gpu, shape, 'checkerboard %dx%dx%d' % (H, W, C))


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('F,C', [(64, 4), (4096, 4), (4100, 3), (16384, 4), (16384, 1)])
def test_chunk_counts_and_tiles_of_many_candidates(gpu, oracle, shape, F, C):
    """1, 64, 65 and 256 chunks: one, one, two and four waves hold directory cells.  From 4 096 faces on, every tile of the 70 x 90 frame has several rounds of candidates."""
    assert (F + 63) // 64 in (1, 64, 65, 256)
    s = scenes.rand_scene(F, 70, 90, C, seed=50 + F % 97, r_lo=0.03, r_hi=0.12)
    want, vis = oracle_side(oracle, s)
    assert np.any(vis >= 0), 'the case wants covered pixels'
    if F == 64:
        assert np.any(vis < 0), 'the case wants uncovered pixels'
    else:
        assert _candidates_per_tile(s) > 2 * V2_CAP, 'the case wants tiles of more than two rounds of candidates'
        assert np.any(vis >= 64 * ((F + 63) // 64 - 1)), 'the case wants a winner from the last chunk'
    check_against_oracle(s, want, vis, oracle, gpu, shape, 'F=%d C=%d' % (F, C))


@pytest.mark.parametrize('shape', SHAPES)
def test_one_workspace_dense_then_sparse_then_dense(gpu, oracle, shape):
    """The ops' cached workspace (same sizes: same block) serves a scene of many rounds per tile, a sparse one and the first
    again: a candidate list, a slot count or shading data left over from the call before would change pixels."""
    dense = scenes.rand_scene(4096, 70, 90, 4, seed=61, r_lo=0.03, r_hi=0.12)
    sparse = scenes.rand_scene(4096, 70, 90, 4, seed=62, r_lo=0.002, r_hi=0.01)
    wd, vd = oracle_side(oracle, dense)
    wsp, vsp = oracle_side(oracle, sparse)
    assert _candidates_per_tile(dense) > 2 * V2_CAP and np.any(vsp >= 0) and np.any(vsp < 0)
    for what, s, want in (('dense', dense, wd), ('sparse after dense', sparse, wsp), ('dense again', dense, wd), ('dense a third time', dense, wd)):
        got = _forward_gpu(s, gpu, shape).cpu().numpy()
        nbad = int(np.sum(got.view(np.uint32) != want.view(np.uint32)))
        assert nbad == 0, '%s: %d of %d pixel values differ from the oracle' % (what, nbad, got.size)
