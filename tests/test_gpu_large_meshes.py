"""GPU parity on meshes of more than 16 384 faces, where the forward pipeline changes (dirt_raster.hip::chunking):

    faces              chunk_faces       nchunk   directory / set-up                             raster
    <= 16 384          64                <= 256   masked cells, setup_kernel_v2 (dirt_forward.hip)   raster_kernel_v2 / raster_kernel (masked)
    16 385 - 65 536    65 - 256          <= 256   start / count cells of 256 bins + "big",         raster_kernel on start / count runs
                                                  setup_kernel<4>, one face per thread
    > 65 536           ceil(F / 256)     256      the same; a thread owns several faces, whose boxes  the same
                                                  go to g.boxes and are re-read in pass 2

chunk_faces = 64 if 64 * 256 >= F else ceil(F / 256); nchunk = ceil(F / chunk_faces).  The face counts below, with
(chunk_faces, nchunk):
    16 384 -> (64, 256)     the control: the last masked count
    16 385 -> (65, 253)     the first start / count count
    20 000 -> (79, 254)
    65 536 -> (256, 256)    the last count where every thread of setup_kernel<4> (256 threads) owns one face
    65 537 -> (257, 256)    the first where thread 0 of a chunk owns two faces (pass 2 re-reads g.boxes)
   200 000 -> (782, 256)    four faces per thread
The start / count bin grid has 256 bins of 32 pixels, or of 64, 128, ... where the frame needs more: 640 x 600 (20 x 19
bins at 32 px) takes 64-pixel bins, 40 x 4096 is exactly 256 bins at 32 px, 40 x 4128 (258) takes 64-pixel bins.

What is asserted is what test_gpu_parity.py::test_forward_bit_exact_and_gradients asserts, at the same tolerance: forward bit
for bit (also through the state-keeping forward), the visibility op equal to the oracle's, grad_background bit for bit,
debug_thingy equal, vertex gradients within parity.TIGHT_TOL of each element's own terms -- for quirk Q1 off and on, through the
forward's state (interleaved accumulators; 'dense' outputs) and statelessly."""
import numpy as np
import pytest
import torch

from dirt_amd import rasterise_ops as ops
from tests import parity, scenes
from tests.test_gpu_parity import TILE_SHAPES

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def chunking(F):
    """dirt_raster.hip::chunking (restated: the docstring's table is computed from it)."""
    chunk = 64 if 64 * 256 >= F else (F + 255) // 256
    return chunk, max(1, (F + chunk - 1) // chunk)


def test_face_counts_land_on_the_regime_edges():
    """(no GPU work) The face counts of this file's cases straddle the two switches of chunking()."""
    assert chunking(16384) == (64, 256) and chunking(16385) == (65, 253) and chunking(20000) == (79, 254)
    assert chunking(65536) == (256, 256) and chunking(65537) == (257, 256) and chunking(200000) == (782, 256)


def _mesh(kind, F, H, W, C, seed):
    if kind == 'small':     # small radii: a few pixels each at these frames
        return scenes.rand_scene(F, H, W, C, seed, 0.001, 0.02)
    if kind == 'grid':      # the shared-vertex grid: high valence, the vertex atomics collide
        return scenes.rand_scene(F, H, W, C, seed, 0.0, 0.0, shared=True)
    if kind == 'large':     # large radii: many faces on the "big" pseudo-bin (a box over more than 4 bins)
        return scenes.rand_scene(F, H, W, C, seed, 0.05, 0.25)
    raise ValueError(kind)


def _check_scene(gpu, oracle, s, H, W, C, tiles, what, debug=True):
    """The assertions of test_forward_bit_exact_and_gradients, plus visibility and the state-fed backward passes; `s` batched."""
    d = {k: _t(s[k], gpu) for k in ('background', 'vertices', 'vertex_colors', 'faces', 'grad_pixels')}
    want = oracle.forward(s['background'], s['vertices'], s['vertex_colors'], s['faces'] if s['faces'].ndim == 3 else
                          np.broadcast_to(s['faces'], (s['vertices'].shape[0],) + s['faces'].shape))
    got = ops._op_rasterise(d['background'], d['vertices'], d['vertex_colors'], d['faces'], H, W, C, flags=tiles).cpu().numpy()
    nbad = int(np.sum(got.view(np.uint32) != want.view(np.uint32)))
    assert nbad == 0, '%s: %d of %d pixel values differ from the oracle' % (what, nbad, got.size)
    faces_b = s['faces'] if s['faces'].ndim == 3 else np.broadcast_to(s['faces'], (s['vertices'].shape[0],) + s['faces'].shape)
    vis = ops._op_visibility(d['vertices'], d['faces'], H, W).cpu().numpy()
    for i in range(vis.shape[0]):
        assert np.array_equal(vis[i], oracle.visibility(s['vertices'][i], faces_b[i], H, W)[0]), '%s: visibility of scene %d' % (what, i)
    for flags in (0, 1):
        ow = oracle.backward(s['vertices'], faces_b, want, s['grad_pixels'], flags=flags, want_debug=debug)
        # stateless (flags 0: with the debug output -- its own kernel instantiation; flags 1: the shape `tiles` pins)
        dbg_on = debug and flags == 0
        gb, gv, gvc, dbg = ops._op_rasterise_grad(d['vertices'], d['faces'], _t(want, gpu), d['grad_pixels'], H, W, C,
                                                  flags=flags | tiles, want_debug=dbg_on)
        assert np.array_equal(gb.cpu().numpy(), ow['grad_background']), '%s flags=%d: grad_background' % (what, flags)
        parity.grads_close(gv, gvc, ow, '%s flags=%d stateless' % (what, flags), tol=parity.TIGHT_TOL)
        if dbg_on:
            assert np.array_equal(dbg.cpu().numpy(), ow['debug_thingy']), '%s: debug_thingy' % what
        # through the forward's state: flags 0 -> 'dense' outputs (DENSE_FROM_STATE), flags 1 -> the state's interleaved accumulators
        px, state = ops._op_rasterise(d['background'], d['vertices'], d['vertex_colors'], d['faces'], H, W, C, flags=tiles, keep_state=True)
        assert np.array_equal(px.cpu().numpy().view(np.uint32), want.view(np.uint32)), '%s: forward with keep_state' % what
        gb, gv, gvc, _ = ops._op_rasterise_grad(d['vertices'], d['faces'], px, d['grad_pixels'], H, W, C, flags=flags | tiles,
                                                state=state, state_outputs='dense' if flags == 0 else True)
        assert np.array_equal(gb.cpu().numpy(), ow['grad_background']), '%s flags=%d: grad_background (state)' % (what, flags)
        parity.grads_close(gv, gvc, ow, '%s flags=%d state' % (what, flags), tol=parity.TIGHT_TOL)


REGIMES = [16384, 16385, 20000, 65536, 65537, 200000]
FRAMES = [(48, 80), (333, 257), (640, 600), (40, 4096), (40, 4128)]   # dense / odd mid-size / > 256 bins / exactly 256 / 258 bins
CHANNELS = [1, 3, 4, 2, 5, 16, 4]   # 1, 3, 4: the CSPEC raster and specialised gradient kernels; 2, 5, 16: generic and strided passes
MESHES = ['small', 'grid', 'large']


def _cases():
    """Every regime meets every tile shape (7 cases each) and every channel count; frames and mesh kinds rotate at other
    periods so that they meet most regimes too.  Large faces stay under 70 000 (beyond, the frame is overdrawn ~10^4 times)."""
    out = []
    for r, F in enumerate(REGIMES):
        for i, tiles in enumerate(TILE_SHAPES):
            C = CHANNELS[(i + r) % len(CHANNELS)]
            H, W = FRAMES[(i + 2 * r) % len(FRAMES)]
            kind = MESHES[(i + r) % len(MESHES)]
            if kind == 'large' and F > 70000:
                kind = 'small'
            out.append(pytest.param(F, H, W, C, kind, tiles.values[0], id='F%d-%dx%d-C%d-%s-%s' % (F, H, W, C, kind, tiles.id)))
    return out


@pytest.mark.parametrize('F,H,W,C,kind,tiles', _cases())
def test_large_mesh_parity(gpu, oracle, F, H, W, C, kind, tiles):
    s = _mesh(kind, F, H, W, C, F % 1000 + 7 * C + H)
    s = {k: (v[None] if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    assert s['faces'].shape[1] == F
    _check_scene(gpu, oracle, s, H, W, C, tiles, 'F=%d %dx%d C=%d %s' % (F, H, W, C, kind))


@pytest.mark.parametrize('n_small,H,W,C,tiles', [
    (40000, 96, 128, 4, 0),          # ~40 000 faces: start / count directory, one face per thread
    (40000, 333, 257, 3, 0x400 | 0x4000),
    (140000, 200, 160, 1, 0x200 | 0x8000),   # ~140 000 faces: several faces per set-up thread
    (140000, 64, 72, 5, 0x600 | 0x2000),
])
def test_large_hostile_meshes(gpu, oracle, n_small, H, W, C, tiles):
    """hostile_scene with tens of thousands of faces: NaN / inf vertices, out-of-range and negative indices, near-plane
    crossings, frame-filling and enormous triangles land at random positions far beyond face 16 384, and the sub-pixel cluster
    puts n_small / 2 faces (20 000 / 70 000) into one tile."""
    s = scenes.hostile_scene(H, W, C, 3 + n_small // 1000, n_small)
    assert s['faces'].shape[0] > 16384
    s = {k: (v[None] if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    _check_scene(gpu, oracle, s, H, W, C, tiles, 'hostile n=%d %dx%d C=%d' % (n_small, H, W, C))


@pytest.mark.parametrize('F,C,shared_faces', [(20000, 3, False), (20000, 4, True), (70000, 1, False), (70000, 16, True)])
def test_large_mesh_batches(gpu, oracle, F, C, shared_faces):
    """B = 3 scenes of a large mesh: [B, F, 3] faces of their own, or one [F, 3] topology for the batch
    (DIRT_FLAG_SHARED_FACES: rasterise_batch with 2-D faces)."""
    H, W = 120, 176
    if shared_faces:
        base = scenes.rand_scene(F, H, W, C, 61, shared=True)
        rng = np.random.default_rng(F + C)
        verts = np.stack([base['vertices'] * (1 + 0.02 * rng.standard_normal(base['vertices'].shape)).astype(np.float32) for _ in range(3)])
        s = dict(vertices=verts.astype(np.float32), faces=base['faces'],
                 vertex_colors=rng.uniform(0, 1, (3,) + base['vertex_colors'].shape).astype(np.float32),
                 background=rng.uniform(0, 1, (3, H, W, C)).astype(np.float32),
                 grad_pixels=rng.standard_normal((3, H, W, C)).astype(np.float32))
    else:
        s = scenes.batch_scene(F, H, W, C, seeds=[71, 72, 73], r_lo=0.001, r_hi=0.03)
    _check_scene(gpu, oracle, s, H, W, C, 0, 'batch F=%d C=%d shared=%s' % (F, C, shared_faces))
    if shared_faces:   # ... and through autograd with the 2-D faces: what the tiled topology gives
        d = {k: _t(s[k], gpu) for k in ('background', 'vertices', 'vertex_colors', 'grad_pixels')}
        tiled = np.ascontiguousarray(np.broadcast_to(s['faces'], (3,) + s['faces'].shape))
        outs = []
        for f in (s['faces'], tiled):
            b_, v_, c_ = (d[k].clone().requires_grad_(True) for k in ('background', 'vertices', 'vertex_colors'))
            px = ops.rasterise_batch(b_, v_, c_, _t(f, gpu))
            px.backward(d['grad_pixels'])
            outs.append((px.detach(), b_.grad, v_.grad, c_.grad))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        ow = oracle.backward(s['vertices'], tiled, outs[1][0].cpu().numpy(), s['grad_pixels'])
        parity.grads_close(outs[0][2], outs[0][3], ow, 'autograd, shared faces', tol=parity.TIGHT_TOL)


def test_big_fuzz_slice(gpu, oracle):
    """A fixed-seed slice of tests/fuzz_parity.py's `big` mode: 16 385 to 250 000 faces, random frames (thin ones up to
    DIRT_MAX_DIM long), channel counts, mesh kinds, batches, tile and gradient-shape flags, with and without the state."""
    from tests import fuzz_parity
    assert fuzz_parity.run(max_cases=24, seed=1618, big=True) == 24
