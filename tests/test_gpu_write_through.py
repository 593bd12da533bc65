"""The outputs that the step's kernels write THROUGH the L2 (dirt_amd/csrc/dirt_device.h: st_off_wt) where
another kind of store can go wrong: its width and its offset (outputs that are slices of larger tensors pre-filled with a NaN of a
known payload: afterwards no element of an output still holds it, every element before and behind the slice still does), frames
of one pixel, with partial tiles in both directions and of 2 x 2 gradient tiles (the halo of a tile is state that another
workgroup wrote), and readers that are not the next launch of the same stream: a second backward over one forward, a torch
kernel on a second stream behind an event, the captured graph of the step replayed.  Pixels, face ids and grad_background bit
for bit against the CPU oracle, vertex gradients by tests/parity.py's rule.

Which kernels write through, and which cases reach them:
  * `pixels` and both state planes: raster_kernel_v2<0, 4, 8> only -- 4 channels, the eight-wave shape, which the library
    picks for 512 to 2048 tiles of 32 x 32 and which both tile flags together pin (LARGE8 below).  Reached by the
    `*-eight-waves*` runs with 4 channels, by the second-backward and second-stream tests (pinned) and by the graph test, whose
    750 x 720 frame (552 tiles) takes that shape by itself.  Small frames without flags render on 16 x 16 tiles
    (dirt_raster.hip), LARGE alone pins the four-wave shape, 1 and 3 channels: all plain stores, run here as the neighbours that
    must not change.
  * `grad_background`: grad_kernel<4>, pairs form (DIRT_FLAG_GRAD_PAIRS, or the library's choice for the small frames here)
    and aliased form (launches of 2048 workgroups and more: test_aliased_form_of_the_gradient_kernel), and grad_kernel_px2<4>
    (DIRT_FLAG_GRAD_PX2; the library's choice at 750 x 720).  The rows form (`*-rows`) and 1 / 3 channels stay plain."""
import functools

import numpy as np
import pytest
import torch

from dirt_amd import _lib, rasterise_ops as ops
from dirt_amd.graphed import GraphedStep
from tests import parity, scenes

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC5A5A5   # a quiet NaN no kernel produces: what the guard bytes and the not-yet-written outputs hold
PAD = 256               # guard elements on either side of an output

LARGE, LARGE8 = _lib.FLAG_TILES_LARGE, _lib.FLAG_TILES_LARGE | _lib.FLAG_TILES_SMALL
# (height, width, faces, their radii): 1 x 1; partial tiles in both directions; 2 x 2 tiles of 32 x 32; 3 x 3 tiles for the pinned raster shapes
FRAMES = {'1x1': (1, 1, 12, 0.8, 1.5), '33x17': (17, 33, 40, 0.05, 0.4), '64x64': (64, 64, 48, 0.05, 0.4), '96x96': (96, 96, 60, 0.05, 0.4),
          '750x720': (720, 750, 60, 0.05, 0.4)}   # 24 x 23 = 552 tiles: the eight-wave shape and the two-pixel gradient kernel by the library's own rules
# (frame, forward flags, backward flags): every frame as the library itself runs it, then the pinned shapes
RUNS = [pytest.param('1x1', 0, 0, id='1x1'), pytest.param('33x17', 0, 0, id='33x17'), pytest.param('64x64', 0, 0, id='64x64'),
        pytest.param('64x64', LARGE, _lib.FLAG_GRAD_ROWS, id='64x64-large-tiles-rows'),
        pytest.param('64x64', LARGE, _lib.FLAG_GRAD_PX2, id='64x64-large-tiles-px2'),
        pytest.param('33x17', LARGE, _lib.FLAG_GRAD_PAIRS, id='33x17-large-tiles-pairs'),
        pytest.param('96x96', LARGE, 0, id='96x96-four-waves'), pytest.param('96x96', LARGE8, _lib.FLAG_GRAD_PAIRS, id='96x96-eight-waves'),
        # the gradient kernel's halo reads state that ANOTHER workgroup wrote through; partial tiles under the written-through stores
        pytest.param('64x64', LARGE8, _lib.FLAG_GRAD_PAIRS, id='64x64-eight-waves-pairs'),
        pytest.param('64x64', LARGE8, _lib.FLAG_GRAD_PX2, id='64x64-eight-waves-px2'),
        pytest.param('33x17', LARGE8, _lib.FLAG_GRAD_PAIRS, id='33x17-eight-waves-pairs'),
        pytest.param('1x1', LARGE8, _lib.FLAG_GRAD_PAIRS, id='1x1-eight-waves-pairs')]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _case(frame, C, empty=False):
    """(batched scene, the oracle's pixels, its backward dict, its face ids), built once and shared; read-only.
    empty: the same mesh moved out of the frame -- an all-background image."""
    import oracle
    oracle.build()
    H, W, F, r_lo, r_hi = FRAMES[frame]
    s = scenes.rand_scene(F, H, W, C, 7 + H, r_lo, r_hi)
    if empty:
        s['vertices'] = s['vertices'].copy()
        s['vertices'][:, 0] += 8.0 * s['vertices'][:, 3]   # NDC x + 8
    b = {k: s[k][None] for k in ('background', 'vertices', 'vertex_colors', 'faces', 'grad_pixels')}
    want = oracle.forward(b['background'], b['vertices'], b['vertex_colors'], b['faces'])
    ow = oracle.backward(b['vertices'], b['faces'], want, b['grad_pixels'], want_mass=True)
    fid = oracle.visibility(s['vertices'], s['faces'], H, W)[0]
    for a in [want, fid] + list(b.values()) + [v for v in ow.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    covered = int((fid >= 0).sum())
    assert (covered == 0) == empty, 'the scene is not what the case claims'
    return b, want, ow, fid


class _Guarded:
    """An output of n 4-byte elements in the middle of a larger tensor filled with NAN_BITS."""

    def __init__(self, shape, dev, dtype=torch.float32):
        self.shape, self.n = shape, int(np.prod(shape))
        self.raw = torch.full((PAD + self.n + PAD,), NAN_BITS, dtype=torch.int32, device=dev)
        self.out = self.raw[PAD:PAD + self.n].view(dtype).view(shape)
        assert self.out.data_ptr() == self.raw.data_ptr() + 4 * PAD and self.out.data_ptr() % 16 == 0

    def ptr(self):
        return self.out.data_ptr()

    def check(self, what):
        raw = self.raw.cpu().numpy()
        assert np.all(raw[:PAD] == NAN_BITS), '%s: bytes BEFORE the output were written' % what
        assert np.all(raw[PAD + self.n:] == NAN_BITS), '%s: bytes BEHIND the output were written' % what
        left = int(np.sum(raw[PAD:PAD + self.n] == NAN_BITS))
        assert left == 0, '%s: %d of %d elements of the output were never written' % (what, left, self.n)
        return raw[PAD:PAD + self.n].reshape(self.shape)


def _step_guarded(b, dev, fwd_flags, bwd_flags):
    """The benchmark's step through the C ABI -- the forward keeps its state and clears the dense vertex gradients in its own
    launch, the backward adds into them -- with every output a slice of a guarded tensor.  Returns the outputs as uint32 /
    float32 numpy arrays: pixels, grad_background, grad_vertices, grad_vertex_colors, face ids."""
    lib = _lib.load()
    d = {k: ops._dense16(_t(v, dev)) for k, v in b.items()}
    B, H, W, C = b['background'].shape
    V, F = b['vertices'].shape[1], b['faces'].shape[1]
    px, gb = _Guarded((B, H, W, C), dev), _Guarded((B, H, W, C), dev)
    gv, gvc = _Guarded((B, V, 4), dev), _Guarded((B, V, C), dev)
    vis = _Guarded((B, H, W), dev, torch.int32)
    stream = ops._stream_handle(dev)
    with ops._on_device(dev):
        ws = torch.empty(lib.dirt_workspace_bytes(B, V, F, H, W, C), dtype=torch.uint8, device=dev)
        _lib.check(lib.dirt_rasterise_forward_train(
            d['background'].data_ptr(), d['vertices'].data_ptr(), d['vertex_colors'].data_ptr(), d['faces'].data_ptr(), px.ptr(),
            gv.ptr(), gvc.ptr(), B, V, F, H, W, C, ws.data_ptr(), ws.numel(), fwd_flags | _lib.FLAG_KEEP_STATE, stream))
        _lib.check(lib.dirt_rasterise_backward(
            d['vertices'].data_ptr(), d['faces'].data_ptr(), px.ptr(), d['grad_pixels'].data_ptr(), gb.ptr(), gv.ptr(), gvc.ptr(), None,
            B, V, F, H, W, C, ws.data_ptr(), ws.numel(), fwd_flags | bwd_flags | _lib.FLAG_REUSE_STATE | _lib.FLAG_OUTPUTS_CLEARED, stream))
        ws1 = ops._workspace(dev, lib.dirt_workspace_bytes(B, V, F, H, W, 1))
        _lib.check(lib.dirt_rasterise_visibility(d['vertices'].data_ptr(), d['faces'].data_ptr(), vis.ptr(), B, V, F, H, W,
                                                 ws1.data_ptr(), ws1.numel(), fwd_flags & _lib.FLAG_TILES_LARGE, stream))
    torch.cuda.synchronize(dev)
    return (px.check('pixels'), gb.check('grad_background'), gv.check('grad_vertices').view(np.float32),
            gvc.check('grad_vertex_colors').view(np.float32), vis.check('face ids'))


def _same_bits(got, want, what):
    want = np.ascontiguousarray(want)
    nbad = int(np.sum(np.ascontiguousarray(got).view(np.uint32) != want.view(np.uint32)))
    assert nbad == 0, '%s: %d of %d values differ from the oracle' % (what, nbad, want.size)


@pytest.mark.parametrize('empty', [False, True], ids=['faces', 'all-background'])
@pytest.mark.parametrize('C', [4, 3, 1])
@pytest.mark.parametrize('frame,fwd_flags,bwd_flags', RUNS)
def test_outputs_exact_and_inside_their_slices(gpu, frame, fwd_flags, bwd_flags, C, empty):
    b, want, ow, fid = _case(frame, C, empty)
    px, gb, gv, gvc, vis = _step_guarded(b, gpu, fwd_flags, bwd_flags)
    what = '%s, %d channels' % (frame, C)
    _same_bits(px, want, what + ' pixels')
    assert np.array_equal(vis[0].view(np.int32), fid), what + ' face ids'
    _same_bits(gb, ow['grad_background'], what + ' grad_background')
    parity.grads_close(gv, gvc, ow, what, tol=parity.TIGHT_TOL)


GRAD_FORMS = [pytest.param(_lib.FLAG_GRAD_PAIRS, id='pairs'), pytest.param(_lib.FLAG_GRAD_PX2, id='px2')]


@pytest.mark.parametrize('grad_form', GRAD_FORMS)
@pytest.mark.parametrize('frame', ['33x17', '64x64'])
def test_second_backward_over_one_forward(gpu, frame, grad_form):
    """4 channels, the eight-wave raster shape pinned: raster_kernel_v2<0, 4, 8> writes `pixels` and both state planes through.
    The first backward adds into the tensors the forward cleared; the second finds nothing cleared for it and clears for
    itself.  Both read that state -- at 64 x 64 across the borders of 2 x 2 tiles -- and write grad_background through
    (grad_kernel<4> pairs form, grad_kernel_px2<4>)."""
    C = 4
    b, want, ow, _ = _case(frame, C, False)
    H, W = want.shape[1:3]
    d = {k: _t(v, gpu) for k, v in b.items()}
    px, state = ops._op_rasterise(d['background'], d['vertices'], d['vertex_colors'], d['faces'], H, W, C, flags=LARGE8, keep_state=True, dense_grads=True)
    _same_bits(px.cpu().numpy(), want, 'pixels')
    first = ops._op_rasterise_grad(d['vertices'], d['faces'], px, d['grad_pixels'], H, W, C, flags=LARGE8 | grad_form, state=state, state_outputs='dense')
    second = ops._op_rasterise_grad(d['vertices'], d['faces'], px, d['grad_pixels'], H, W, C, flags=LARGE8 | grad_form, state=state, state_outputs=False)
    for name, (gb, gv, gvc, _) in (('first', first), ('second', second)):
        _same_bits(gb.cpu().numpy(), ow['grad_background'], '%s backward grad_background' % name)
        parity.grads_close(gv, gvc, ow, '%s backward' % name, tol=parity.TIGHT_TOL)


@pytest.mark.parametrize('grad_form', GRAD_FORMS)
def test_read_by_a_torch_kernel_on_a_second_stream(gpu, grad_form):
    """What raster_kernel_v2<0, 4, 8> (pinned) and grad_kernel<4> / grad_kernel_px2<4> wrote through is read by a kernel that
    is not theirs, on another stream, ordered by an event only."""
    C = 4
    b, want, ow, _ = _case('64x64', C, False)
    H, W = want.shape[1:3]
    d = {k: _t(v, gpu) for k, v in b.items()}
    side = torch.cuda.Stream(device=gpu)
    px, state = ops._op_rasterise(d['background'], d['vertices'], d['vertex_colors'], d['faces'], H, W, C, flags=LARGE8, keep_state=True, dense_grads=True)
    gb, gv, gvc, _ = ops._op_rasterise_grad(d['vertices'], d['faces'], px, d['grad_pixels'], H, W, C, flags=LARGE8 | grad_form, state=state, state_outputs='dense')
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        side.wait_event(done)
        copies = [t + 0.0 for t in (px, gb, gv, gvc)]   # (x + 0.0 keeps every bit of a value that is not -0.0 ...)
        raw = [t.view(torch.int32).clone() for t in (px, gb)]   # (... and these keep all of them)
    side.synchronize()
    _same_bits(raw[0].cpu().numpy(), want, 'pixels on the second stream')
    _same_bits(raw[1].cpu().numpy(), ow['grad_background'], 'grad_background on the second stream')
    assert np.array_equal(copies[0].cpu().numpy(), want) and np.array_equal(copies[1].cpu().numpy(), ow['grad_background'])
    parity.grads_close(copies[2], copies[3], ow, 'second stream', tol=parity.TIGHT_TOL)


def test_graphed_step_replayed(gpu):
    """The step at 750 x 720 x 4 -- 552 tiles: the library itself picks raster_kernel_v2<0, 4, 8> and grad_kernel_px2<4>, every
    written-through store of the step in one launch chain -- eager, then captured (GraphedStep, which takes no flags) and
    replayed three times: pixels and grad_background bit-identical to the eager call and to the oracle."""
    C = 4
    b, want, ow, _ = _case('750x720', C, False)
    H, W = want.shape[1:3]
    d = {k: _t(v, gpu) for k, v in b.items()}
    px, state = ops._op_rasterise(d['background'], d['vertices'], d['vertex_colors'], d['faces'], H, W, C, keep_state=True, dense_grads=True)
    gb, gv, gvc, _ = ops._op_rasterise_grad(d['vertices'], d['faces'], px, d['grad_pixels'], H, W, C, state=state, state_outputs='dense')
    eager_px, eager_gb = px.cpu().numpy(), gb.cpu().numpy()
    _same_bits(eager_px, want, 'eager pixels')
    _same_bits(eager_gb, ow['grad_background'], 'eager grad_background')
    parity.grads_close(gv, gvc, ow, 'eager', tol=parity.TIGHT_TOL)
    step = GraphedStep(d['background'], d['vertices'], d['vertex_colors'], d['faces'], grad_pixels=d['grad_pixels'])
    for i in range(3):
        for t in (step.pixels, step.grads[0]):
            t.view(torch.int32).fill_(NAN_BITS)   # a replay has to write all of it again
        pixels, grads = step()
        torch.cuda.synchronize(gpu)
        _same_bits(pixels.cpu().numpy(), eager_px, 'replay %d pixels' % i)
        _same_bits(grads[0].cpu().numpy(), eager_gb, 'replay %d grad_background' % i)
        parity.grads_close(grads[1], grads[2], ow, 'replay %d' % i, tol=parity.TIGHT_TOL)


def test_aliased_form_of_the_gradient_kernel(gpu):
    """Four copies of the 750 x 720 scene in one launch: 2208 workgroups, where the library picks grad_kernel<4>'s aliased form
    (from 2048 on), which writes grad_background through; the forward of such a launch is the four-wave shape: plain stores."""
    C, B = 4, 4
    b, want, ow, _ = _case('750x720', C, False)
    H, W = want.shape[1:3]
    d = {k: _t(np.repeat(v, B, axis=0), gpu) for k, v in b.items()}
    px, state = ops._op_rasterise(d['background'], d['vertices'], d['vertex_colors'], d['faces'], H, W, C, keep_state=True, dense_grads=True)
    gb, gv, gvc, _ = ops._op_rasterise_grad(d['vertices'], d['faces'], px, d['grad_pixels'], H, W, C, state=state, state_outputs='dense')
    px, gb = px.cpu().numpy(), gb.cpu().numpy()
    for i in range(B):
        _same_bits(px[i:i + 1], want, 'scene %d pixels' % i)
        _same_bits(gb[i:i + 1], ow['grad_background'], 'scene %d grad_background' % i)
        parity.grads_close(gv[i:i + 1], gvc[i:i + 1], ow, 'scene %d' % i, tol=parity.TIGHT_TOL)
