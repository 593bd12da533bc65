"""Randomised parity sweep on an MI355X box: random frame sizes, channel counts, meshes (split / shared / hostile),
kernel tile shapes and flags; every case compares the HIP path with the CPU oracle (forward
and visibility bit for bit, gradients per element within 5e-6 (parity.TIGHT_TOL; the specification says 1e-4) of the L1 mass of their terms, non-finite values in the same
places: tests/parity.py).  A fixed-seed slice of it runs under pytest (tests/test_gpu_configs.py); as a script it is open-ended (a time budget).
Two opt-in modes draw their own cases: `big` -- meshes of 16 385 to 250 000 faces, where the forward pipeline switches to the
start / count bin directory (forward, visibility and gradients checked; slice: tests/test_gpu_large_meshes.py) -- and `stream` --
4-channel frames whose sides are multiples of 32, with the reserved bit DIRT_FLAG_GRAD_STREAM set, which must change nothing
(slice: tests/test_gpu_grad_stream.py).
usage: python tests/fuzz_parity.py [seconds] [seed] [hostile|big|stream]   (`hostile`: mostly hostile geometry, larger frames)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import oracle  # noqa: E402
from dirt_amd import _lib, rasterise_ops as ops  # noqa: E402
from tests import scenes  # noqa: E402
from tests import parity  # noqa: E402


def _draw_default(rng, hard, max_dim):
    """One case of the default sweep (frames up to 400 / 700 pixels, up to ~4 000 faces).  The order of the draws is the
    sweep's record: test_fuzz_parity_slice reruns exactly these cases."""
    top = max_dim or (700 if hard else 400)
    H, W = int(rng.integers(1, top)), int(rng.integers(1, top))
    C = int(rng.choice([1, 2, 3, 4, 5, 6, 7, 8, 10, 16]))
    kind = rng.choice(['split', 'shared', 'hostile', 'tiny'], p=[0.1, 0.1, 0.7, 0.1] if hard else None)
    seed_ = int(rng.integers(0, 1 << 30))
    if kind == 'hostile':
        s = scenes.hostile_scene(H, W, C, seed_, int(rng.integers(10, 1500)))
    elif kind == 'tiny':
        s = scenes.rand_scene(int(rng.integers(1, 4000)), H, W, C, seed_, 0.001, 0.02)
    else:
        s = scenes.rand_scene(int(rng.integers(1, 3000)), H, W, C, seed_, float(rng.uniform(0.005, 0.1)), float(rng.uniform(0.1, 0.8)), kind == 'shared')
    flags = int(rng.choice([0, 0x200, 0x400, 0x600])) | int(rng.choice([0, 1])) | int(rng.choice([0, 0x1000, 0x2000, 0x4000, 0x8000, 0x8000, 0x10000]))
    b = {k: v[None] for k, v in s.items() if isinstance(v, np.ndarray)}
    if kind in ('split', 'shared') and rng.random() < 0.4:  # a batch of scenes of the same sizes
        B = int(rng.integers(2, 4))
        F = b['faces'].shape[1]
        bs = scenes.batch_scene(F, H, W, C, [seed_ + i for i in range(B)], r_lo=0.01, r_hi=0.3, shared=(kind == 'shared'))
        b = {k: bs[k] for k in ('background', 'vertices', 'vertex_colors', 'faces', 'grad_pixels')}
    use_state = rng.random() < 0.5  # the autograd path: the forward keeps its state, the backward consumes it
    return b, H, W, C, kind, seed_, flags, use_state


BIG_FACES = (16385, 250000)   # the `big` mode's face counts: past the masked directory (chunking() in dirt_raster.hip: F > 16 384)


def _draw_big(rng, max_dim):
    """One case of the large-mesh sweep: 16 385 to 250 000 faces (the start / count directory, chunks of 65 to 977 faces,
    threads owning several faces past 65 536), frames of up to 700 pixels or thin ones up to `max_dim` (<= DIRT_MAX_DIM) long."""
    if rng.random() < 0.15:   # a thin frame: up to DIRT_MAX_DIM along one side
        a, b_ = int(rng.integers(1, 48)), int(rng.integers(700, (max_dim or _MAX_DIM) + 1))
        H, W = (a, b_) if rng.random() < 0.5 else (b_, a)
    else:
        H, W = int(rng.integers(1, 700)), int(rng.integers(1, 700))
    C = int(rng.choice([1, 2, 3, 4, 5, 16]))
    kind = rng.choice(['split', 'shared', 'hostile', 'tiny', 'large'])
    seed_ = int(rng.integers(0, 1 << 30))
    F = int(np.exp(rng.uniform(np.log(BIG_FACES[0]), np.log(BIG_FACES[1]))))
    if kind == 'hostile':
        s = scenes.hostile_scene(H, W, C, seed_, F)
    elif kind == 'tiny':
        s = scenes.rand_scene(F, H, W, C, seed_, 0.0005, 0.01)
    elif kind == 'large':   # large faces (many on the "big" pseudo-bin): fewer of them, or the frame is overdrawn thousands of times
        s = scenes.rand_scene(min(F, 40000), H, W, C, seed_, 0.05, 0.3)
    else:
        s = scenes.rand_scene(F, H, W, C, seed_, 0.001, float(rng.uniform(0.005, 0.03)), kind == 'shared')
    flags = int(rng.choice([0, 0x200, 0x400, 0x600])) | int(rng.choice([0, 1])) | int(rng.choice([0, 0x1000, 0x2000, 0x4000, 0x8000, 0x10000]))
    b = {k: v[None] for k, v in s.items() if isinstance(v, np.ndarray)}
    if kind in ('split', 'shared') and rng.random() < 0.25:
        B = int(rng.integers(2, 4))
        bs = scenes.batch_scene(b['faces'].shape[1], H, W, C, [seed_ + i for i in range(B)], r_lo=0.001, r_hi=0.02, shared=(kind == 'shared'))
        b = {k: bs[k] for k in ('background', 'vertices', 'vertex_colors', 'faces', 'grad_pixels')}
    use_state = rng.random() < 0.5
    return b, H, W, C, kind, seed_, flags, use_state


STREAM_SIDES = (32, 64, 96, 128, 160, 192, 256, 320)


def _draw_stream(rng, sizes=STREAM_SIDES):
    """One case of the `stream` sweep: the reserved bit DIRT_FLAG_GRAD_STREAM set (accepted and ignored: the library's own
    kernel choice runs) on frames whose sides are multiples of 32, 4 channels, every mesh kind, batches, quirk Q1 both ways,
    with and without the forward's state."""
    H, W, C = int(rng.choice(sizes)), int(rng.choice(sizes)), 4
    kind = rng.choice(['split', 'shared', 'hostile', 'tiny'])
    seed_ = int(rng.integers(0, 1 << 30))
    if kind == 'hostile':
        s = scenes.hostile_scene(H, W, C, seed_, int(rng.integers(10, 1500)))
    elif kind == 'tiny':
        s = scenes.rand_scene(int(rng.integers(1, 4000)), H, W, C, seed_, 0.001, 0.02)
    else:
        s = scenes.rand_scene(int(rng.integers(1, 3000)), H, W, C, seed_, float(rng.uniform(0.005, 0.1)), float(rng.uniform(0.1, 0.8)), kind == 'shared')
    q1 = int(rng.choice([0, 1]))
    b = {k: v[None] for k, v in s.items() if isinstance(v, np.ndarray)}
    if kind in ('split', 'shared') and rng.random() < 0.4:
        B = int(rng.integers(2, 4))
        F = b['faces'].shape[1]
        bs = scenes.batch_scene(F, H, W, C, [seed_ + i for i in range(B)], r_lo=0.01, r_hi=0.3, shared=(kind == 'shared'))
        b = {k: bs[k] for k in ('background', 'vertices', 'vertex_colors', 'faces', 'grad_pixels')}
    use_state = rng.random() < 0.5
    return b, H, W, C, kind, seed_, _lib.FLAG_GRAD_STREAM | q1, use_state


_MAX_DIM = 16384   # DIRT_MAX_DIM (include/dirt_hip.h)


def run(budget=None, max_cases=None, seed=0, hard=False, max_dim=None, failures=None, big=False, stream=False):
    """Random cases until `budget` seconds have passed or `max_cases` are done; returns the number of cases.
    `failures`: a list to collect mismatches in instead of raising at the first (the open-ended sweep).
    `big`: meshes of 16 385 to 250 000 faces (_draw_big); `stream`: the reserved-bit sweep (_draw_stream)."""
    rng = np.random.default_rng(seed)
    dev = torch.device('cuda', 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t0, n = time.time(), 0
    while (budget is None or time.time() - t0 < budget) and (max_cases is None or n < max_cases):
        if stream:
            b, H, W, C, kind, seed_, flags, use_state = _draw_stream(rng)
        elif big:
            b, H, W, C, kind, seed_, flags, use_state = _draw_big(rng, max_dim)
        else:
            b, H, W, C, kind, seed_, flags, use_state = _draw_default(rng, hard, max_dim)
        want = oracle.forward(b['background'], b['vertices'], b['vertex_colors'], b['faces'])
        fwd_flags = 0 if stream else flags & ~1
        got = ops._op_rasterise(t(b['background']), t(b['vertices']), t(b['vertex_colors']), t(b['faces']), H, W, C, flags=fwd_flags,
                                keep_state=use_state)
        got, state = got if use_state else (got, None)
        tag = (kind, b['vertices'].shape[0], b['faces'].shape[1], H, W, C, seed_, hex(flags), use_state)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), ('forward', tag)
        if big:   # (the visibility op: what deferred shading renders its G-buffer with)
            vis = ops._op_visibility(t(b['vertices']), t(b['faces']), H, W).cpu().numpy()
            for i in range(vis.shape[0]):
                assert np.array_equal(vis[i], oracle.visibility(b['vertices'][i], b['faces'][i], H, W)[0]), ('visibility', i, tag)
        ow = oracle.backward(b['vertices'], b['faces'], want, b['grad_pixels'], flags=flags & 1, want_mass=True)
        gb, gv, gvc, _ = ops._op_rasterise_grad(t(b['vertices']), t(b['faces']), t(want), t(b['grad_pixels']), H, W, C, flags=flags, state=state)
        assert np.array_equal(gb.cpu().numpy(), ow['grad_background']), ('grad_background', tag)
        try:
            parity.grads_close(gv, gvc, ow, str(tag), tol=parity.TIGHT_TOL)
        except AssertionError as e:
            if failures is None:
                raise
            failures.append(str(e))
        n += 1
    return n


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    t0 = time.time()
    failures = []
    mode = sys.argv[3] if len(sys.argv) > 3 else ''
    n = run(budget=budget, seed=int(sys.argv[2]) if len(sys.argv) > 2 else 0, hard=mode == 'hostile', failures=failures,
            big=mode == 'big', stream=mode == 'stream')
    for f in failures:
        print('MISMATCH', f)
    print('fuzz_parity: %d random cases in %.0f s, forward / visibility / grad_background bit-exact in all, %d gradient mismatches'
          % (n, time.time() - t0, len(failures)))
    if failures:
        sys.exit(1)


if __name__ == '__main__':
    main()
