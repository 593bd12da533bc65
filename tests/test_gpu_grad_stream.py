"""DIRT_FLAG_GRAD_STREAM is a reserved bit: the library accepts it and ignores it (the kernel it once selected was removed).
Every case here sets it and checks the backward against the CPU oracle at parity.TIGHT_TOL per element, grad_background
(and pixels) bit for bit, in all three output forms: that pins that the bit changes nothing.  The cases also cover the
default kernel choice on K3, K3-2048, batches, shared faces, 80 000 faces, the quirk-Q1 right border and misaligned views."""
import numpy as np
import pytest
import torch

from dirt_amd import _lib, rasterise_ops as ops
from tests import parity, scenes

pytestmark = pytest.mark.gpu

STREAM = _lib.FLAG_GRAD_STREAM


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check(gpu, oracle, s, H, W, C, what, q1_modes=(0, 1), forms=('stateless', 'dense', 'state'), want_debug=False):
    """Forward bit for bit, then the backward with STREAM | q1 in each output form: stateless, the state's 'dense' outputs
    (DENSE_FROM_STATE), the state's interleaved accumulators (gv_stride 8: views of the state)."""
    d = {k: _t(s[k], gpu) for k in ('background', 'vertices', 'vertex_colors', 'faces', 'grad_pixels')}
    faces_b = s['faces'] if s['faces'].ndim == 3 else np.ascontiguousarray(np.broadcast_to(s['faces'], (s['vertices'].shape[0],) + s['faces'].shape))
    want = oracle.forward(s['background'], s['vertices'], s['vertex_colors'], faces_b)
    for q1 in q1_modes:
        ow = oracle.backward(s['vertices'], faces_b, want, s['grad_pixels'], flags=q1, want_debug=want_debug)
        for form in forms:
            state = None
            if form != 'stateless':
                px, state = ops._op_rasterise(d['background'], d['vertices'], d['vertex_colors'], d['faces'], H, W, C, keep_state=True)
                assert np.array_equal(px.cpu().numpy().view(np.uint32), want.view(np.uint32)), what + ': forward'
            else:
                px = ops._op_rasterise(d['background'], d['vertices'], d['vertex_colors'], d['faces'], H, W, C)
                assert np.array_equal(px.cpu().numpy().view(np.uint32), want.view(np.uint32)), what + ': forward'
            gb, gv, gvc, dbg = ops._op_rasterise_grad(d['vertices'], d['faces'], px, d['grad_pixels'], H, W, C, flags=STREAM | q1,
                                                      state=state, want_debug=want_debug and form == 'stateless',
                                                      state_outputs={'stateless': True, 'dense': 'dense', 'state': True}[form])
            if form == 'state':
                assert gv.stride(1) == 8, 'expected views of the interleaved accumulators'
            if form == 'dense':
                assert gv.is_contiguous() and gvc.is_contiguous()
            tag = '%s q1=%d %s' % (what, q1, form)
            assert np.array_equal(gb.cpu().numpy().view(np.uint32), ow['grad_background'].view(np.uint32)), tag + ': grad_background'
            parity.grads_close(gv, gvc, ow, tag, tol=parity.TIGHT_TOL)
            if want_debug and form == 'stateless':
                assert np.array_equal(dbg.cpu().numpy(), ow['debug_thingy']), tag + ': debug_thingy'


def test_stream_fuzz_slice(gpu, oracle):
    """A fixed-seed slice of tests/fuzz_parity.py's `stream` mode (the reserved bit set): sides multiples of 32 up to 320,
    4 channels, split / shared / hostile / tiny meshes, batches, Q1 both ways, with and without the state."""
    from tests import fuzz_parity
    assert fuzz_parity.run(max_cases=150, seed=4242, stream=True) == 150


@pytest.mark.parametrize('config', ['K3', 'K3-2048'])
def test_stream_full_size(gpu, oracle, config):
    """The BASELINE scenes at full size (10 000 faces at 1024^2 and 2048^2), in each of the three output forms."""
    s = {k: (v[None] if isinstance(v, np.ndarray) else v) for k, v in scenes.config_scene(config).items()}
    H, W, C = s['height'], s['width'], s['channels']
    _check(gpu, oracle, s, H, W, C, config)


def test_stream_batch(gpu, oracle):
    s = scenes.batch_scene(3000, 256, 256, 4, seeds=[91, 92, 93, 94], r_lo=0.005, r_hi=0.08)
    _check(gpu, oracle, s, 256, 256, 4, 'batch of 4')


def test_stream_shared_faces(gpu, oracle):
    """One [F, 3] topology for a batch of 3 (DIRT_FLAG_SHARED_FACES)."""
    base = scenes.rand_scene(2500, 192, 160, 4, 95, shared=True)
    rng = np.random.default_rng(96)
    s = dict(vertices=np.stack([base['vertices'] * (1 + 0.03 * rng.standard_normal(base['vertices'].shape)) for _ in range(3)]).astype(np.float32),
             faces=base['faces'], vertex_colors=rng.uniform(0, 1, (3,) + base['vertex_colors'].shape).astype(np.float32),
             background=rng.uniform(0, 1, (3, 192, 160, 4)).astype(np.float32),
             grad_pixels=rng.standard_normal((3, 192, 160, 4)).astype(np.float32))
    _check(gpu, oracle, s, 192, 160, 4, 'shared faces')


@pytest.mark.parametrize('W', [32, 64, 96])
def test_stream_right_border_alias_taps(gpu, oracle, W):
    """Quirk Q1 at the right image border (as test_gpu_parity.py::test_right_border_alias_taps, with H and W multiples of 32 and
    the reserved bit set): the aliased channels of the last columns lie in the next row / scene / past the end, which the
    gradient kernels re-read; large faces so that many border pixels are interior and decide their axis."""
    H = 256
    s = scenes.batch_scene(120, H, W, 4, seeds=[181 + W, 182 + W], r_lo=0.05, r_hi=0.4)
    _check(gpu, oracle, s, H, W, 4, 'right border W=%d' % W, q1_modes=(0,), forms=('stateless', 'dense'))


def test_stream_large_mesh(gpu, oracle):
    """More than 65 536 faces (the set-up threads own several faces each): the backward on that state, the reserved bit set."""
    s = {k: (v[None] if isinstance(v, np.ndarray) else v) for k, v in scenes.rand_scene(80000, 320, 384, 4, 97, 0.001, 0.02).items()}
    _check(gpu, oracle, s, 320, 384, 4, '80 000 faces')


@pytest.mark.parametrize('H,W,C,debug', [
    (100, 128, 4, False),    # H not a multiple of 32
    (96, 150, 4, False),     # W not a multiple of 32
    (128, 128, 3, False),    # 3 channels
    (128, 96, 4, True),      # the debug output
])
def test_stream_flag_falls_back(gpu, oracle, H, W, C, debug):
    """The reserved bit set on frames of other shapes -- sides not multiples of 32, 3 channels, the debug output: the results
    are the oracle's."""
    s = scenes.batch_scene(900, H, W, C, seeds=[41, 42], r_lo=0.01, r_hi=0.2)
    _check(gpu, oracle, s, H, W, C, 'fall-back %dx%dx%d debug=%s' % (H, W, C, debug), forms=('stateless', 'dense'), want_debug=debug)


def test_stream_flag_with_misaligned_views(gpu, oracle):
    """`pixels` and `grad_pixels` that start one float into their buffers (not 16-byte aligned; the wrapper copies them, as
    test_misaligned_views_are_accepted) and vertex / face views x[1:] of a batch, through the backward with the reserved bit."""
    s = scenes.batch_scene(60, 32, 32, 4, seeds=[1, 2, 3], r_lo=0.1, r_hi=0.5)
    t = {k: _t(s[k], gpu) for k in ('background', 'vertices', 'vertex_colors', 'faces', 'grad_pixels')}
    pbuf = torch.zeros(2 * 32 * 32 * 4 + 1, device=gpu)
    want = oracle.forward(s['background'][1:], s['vertices'][1:], s['vertex_colors'][1:], s['faces'][1:])
    pbuf[1:] = _t(want.reshape(-1), gpu)
    px = pbuf[1:].view(2, 32, 32, 4)
    gbuf = torch.zeros(2 * 32 * 32 * 4 + 1, device=gpu)
    gbuf[1:] = t['grad_pixels'][1:].reshape(-1)
    gp = gbuf[1:].view(2, 32, 32, 4)
    v = t['vertices'][1:]
    assert px.data_ptr() % 16 != 0 and gp.data_ptr() % 16 != 0
    for q1 in (0, 1):
        ow = oracle.backward(s['vertices'][1:], s['faces'][1:], want, s['grad_pixels'][1:], flags=q1, want_mass=True)
        gb, gv, gvc, _ = ops._op_rasterise_grad(v, t['faces'][1:], px, gp, 32, 32, 4, flags=STREAM | q1)
        assert np.array_equal(gb.cpu().numpy(), ow['grad_background'])
        parity.grads_close(gv, gvc, ow, 'misaligned q1=%d' % q1, tol=parity.TIGHT_TOL)
