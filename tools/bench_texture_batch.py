"""GPU box: a texture per scene in one launch (dirt_texture_*_batch*) against the only route there was before, a loop of B
calls of the single-texture entry points on the same data.  The C-ABI calls alone are timed with HIP events, after warm-up;
per configuration and pass the two routes alternate in one process, `REPS` timings each of as many calls as fill `WINDOW_MS`
(the same count for both routes), and the median and the spread (min .. max) of each are reported.  The (u, v) field is what a
G-buffer holds -- smooth, rotated, `scale` texture tiles across the frame, another angle per scene -- read in place from
channels 1:3 of a 6-channel buffer, the mask from channel 0.  Passes: forward and backward, 'bilinear' and 'trilinear' (level of detail from the footprint), and for
'trilinear' the pyramid build and the collapse.
usage: python tools/bench_texture_batch.py [json path]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from dirt_amd import _lib, rasterise_ops as _ops, texture  # noqa: E402

# scenes, frame, texture, texture tiles across the frame
CONFIGS = [(64, 256, 256, 128, 128, 3, 1.0), (8, 1024, 1024, 512, 512, 3, 1.0), (8, 512, 512, 2048, 2048, 3, 1.0)]
REPS, WINDOW_MS, CG = 15, 20.0, 6
out_path = next((a for a in sys.argv[1:] if a.endswith('.json')), None)
dev = torch.device('cuda:0')
lib = _lib.load()
stream = _ops._stream_handle(dev)


def once(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3   # us


def compare(batch, loop):
    """-> {'batch_us', 'loop_us'}: median and [min, max] of REPS alternating timings."""
    for _ in range(3):
        batch(), loop()
    calls = int(min(400, max(5, WINDOW_MS * 1e3 / once(batch, 5))))
    tb, tl = [], []
    for _ in range(REPS):
        tb.append(once(batch, calls))
        tl.append(once(loop, calls))
    stat = lambda t: {'median': float(np.median(t)), 'min': float(min(t)), 'max': float(max(t))}
    return {'calls_per_timing': calls, 'batch_us': stat(tb), 'loop_us': stat(tl), 'loop_over_batch': float(np.median(tl) / np.median(tb))}


def ok(rc):
    assert rc == 0, lib.dirt_texture_last_error()


rows = []
for B, H, W, Ht, Wt, Ct, scale in CONFIGS:
    rng = np.random.default_rng(0)
    tex = torch.from_numpy(rng.uniform(0, 1, (B, Ht, Wt, Ct)).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.standard_normal((B, H, W, Ct)).astype(np.float32)).to(dev)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing='ij')
    gbuf = np.ones((B, H, W, CG), np.float32)
    for b in range(B):
        c, s = np.cos(0.2 + 0.05 * b), np.sin(0.2 + 0.05 * b)
        gbuf[b, ..., 1] = (c * xs / W + s * ys / H) * scale + 0.13
        gbuf[b, ..., 2] = (-s * xs / W + c * ys / H) * scale + 0.41
    gb = torch.from_numpy(gbuf).to(dev)
    n = H * W
    levels, floats, _ = texture._mip_geometry(Ht, Wt, Ct, None)
    out, gt = torch.empty((B, H, W, Ct), device=dev), torch.empty_like(tex)
    guv = torch.empty((B, H, W, 2), device=dev)
    pyr, scratch = torch.empty((B, floats), device=dev), torch.empty((B, floats), device=dev)
    P = lambda t, b=0, stride=0: t.data_ptr() + 4 * b * stride      # scene b of a tensor whose scenes lie `stride` floats apart
    uv0, m0 = gb.data_ptr() + 4, gb.data_ptr()
    tex_s, px_s, gb_s = Ht * Wt * Ct, n * Ct, n * CG
    ok(lib.dirt_texture_mip_build_batch(P(tex), P(pyr), B, Ht, Wt, Ct, levels, stream))
    passes = {
        'bilinear forward': (
            lambda: ok(lib.dirt_texture_sample_batch_forward(P(tex), uv0, P(out), B, n, Ht, Wt, Ct, CG, 0, stream)),
            lambda: [ok(lib.dirt_texture_sample_forward(P(tex, b, tex_s), uv0 + 4 * b * gb_s, P(out, b, px_s), n, Ht, Wt, Ct, CG, 0, stream)) for b in range(B)]),
        'bilinear backward': (
            lambda: ok(lib.dirt_texture_sample_batch_backward_image(P(tex), uv0, P(g), P(gt), P(guv), B, H, W, Ht, Wt, Ct, CG, 2, 0, stream)),
            lambda: [ok(lib.dirt_texture_sample_backward_image(P(tex, b, tex_s), uv0 + 4 * b * gb_s, P(g, b, px_s), P(gt, b, tex_s), P(guv, b, 2 * n), H, W,
                                                              Ht, Wt, Ct, CG, 2, 0, stream)) for b in range(B)]),
        'pyramid build': (
            lambda: ok(lib.dirt_texture_mip_build_batch(P(tex), P(pyr), B, Ht, Wt, Ct, levels, stream)),
            lambda: [ok(lib.dirt_texture_mip_build(P(tex, b, tex_s), P(pyr, b, floats), Ht, Wt, Ct, levels, stream)) for b in range(B)]),
        'pyramid collapse': (
            lambda: ok(lib.dirt_texture_mip_collapse_batch(P(scratch), P(gt), B, Ht, Wt, Ct, levels, stream)),
            lambda: [ok(lib.dirt_texture_mip_collapse(P(scratch, b, floats), P(gt, b, tex_s), Ht, Wt, Ct, levels, stream)) for b in range(B)]),
        'trilinear forward': (
            lambda: ok(lib.dirt_texture_sample_mip_batch_forward(P(pyr), uv0, None, m0, P(out), B, H, W, H, Ht, Wt, Ct, levels, CG, CG, 0.0, 0, stream)),
            lambda: [ok(lib.dirt_texture_sample_mip_forward(P(pyr, b, floats), uv0 + 4 * b * gb_s, None, m0 + 4 * b * gb_s, P(out, b, px_s), H, W, H, Ht, Wt, Ct,
                                                           levels, CG, CG, 0.0, 0, stream)) for b in range(B)]),
        'trilinear backward (clear, tiles, collapse)': (
            lambda: ok(lib.dirt_texture_sample_mip_batch_backward(P(pyr), uv0, None, m0, P(g), P(scratch), P(gt), P(guv), None, B, H, W, H, Ht, Wt, Ct, levels,
                                                                  CG, 2, CG, 0.0, 0, stream)),
            lambda: [ok(lib.dirt_texture_sample_mip_backward(P(pyr, b, floats), uv0 + 4 * b * gb_s, None, m0 + 4 * b * gb_s, P(g, b, px_s), P(scratch, b, floats),
                                                            P(gt, b, tex_s), P(guv, b, 2 * n), None, H, W, H, Ht, Wt, Ct, levels, CG, 2, CG, 0.0, 0, stream))
                     for b in range(B)]),
    }
    for name, (batch, loop) in passes.items():
        r = {'scenes': B, 'frame': [H, W], 'texture': [Ht, Wt, Ct], 'pass': name}
        r.update(compare(batch, loop))
        rows.append(r)
        print(json.dumps(r))
if out_path:
    json.dump({'workload': 'a texture per scene: one batched C-ABI call against a loop of single-texture calls, (u, v) and mask in place from a '
                           '6-channel G-buffer; us per call of the whole batch, median and [min, max] of %d alternating timings of about %g ms each' % (REPS, WINDOW_MS),
               'results': rows}, open(out_path, 'w'), indent=1)
