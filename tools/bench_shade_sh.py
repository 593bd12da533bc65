"""The fused spherical-harmonic G-buffer lighting (dirt_amd.shading.shade_gbuffer_sh) against the float32 torch composition of
the same shader (lighting.spherical_harmonics, the mask composite, the clamp), timed with HIP events after warm-up, in one
process, the two legs alternating (the method of tools/bench_shade.py):
  shader_WxHxC    forward + backward on a resident G-buffer with gradients to the G-buffer, the coefficients and the
                  background, at 640x480x10 and 2048x2048x16;
  tensor_WxHx6    the same with the colours in a tensor of their own beside a 6-channel G-buffer (mask, normals, two unused).
Every figure is the median over `repeats` blocks of `steps` steps, with the spread (min .. max) of the blocks.  The condition:
the fused leg is faster than the torch leg in every row by more than the torch leg's own spread.
usage (GPU box): python tools/bench_shade_sh.py [steps] [repeats]     (prints one JSON line, writes profiles/shade_sh.json)
                 python tools/bench_shade_sh.py --trace               (three steps of every fused leg and of the one-light
                                                                       shade_gbuffer at the same shapes, for a kernel trace)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from dirt_amd import lighting, shading  # noqa: E402
from bench_shade import time_alternating  # noqa: E402

KW = dict(band_scale=lighting.SH_LAMBERT, normalize=True)


def torch_shader(gbuffer, colors, table, background):
    mask, normals = gbuffer[..., :1], gbuffer[..., 7:10] if colors is None else gbuffer[..., 1:4]
    colors = gbuffer[..., 4:7] if colors is None else colors
    lit = lighting.spherical_harmonics(normals, colors, table, **KW)
    return torch.clamp(lit * mask + background * (1. - mask), 0., 1.)


def fused_shader(gbuffer, colors, table, background):
    if colors is None:
        return shading.shade_gbuffer_sh(gbuffer, table, colors=4, normals=7, mask=0, background=background, **KW)
    return shading.shade_gbuffer_sh(gbuffer, table, colors=colors, normals=1, mask=0, background=background, **KW)


def one_light_shader(gbuffer):
    return shading.shade_gbuffer(gbuffer, [shading.diffuse_directional_light(torch.tensor([0.6, -0.64, -0.48], device=gbuffer.device,
                                                                                          requires_grad=True), (1., 0., 0.), False)],
                                 colors=4, normals=7, mask=0, ambient=(0.2, 0.2, 0.2), background=(0., 0., 0.3))


def inputs(dev, rng, h, w, c, tensor):
    g = torch.rand(h, w, c, device=dev)
    g[..., 0] = (g[..., 0] < 0.7).float()
    g.requires_grad_(True)
    col = torch.rand(h, w, 3, device=dev, requires_grad=True) if tensor else None
    d = torch.from_numpy(rng.standard_normal((h, w, 3)).astype(np.float32)).to(dev)
    return g, col, d


def main():
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    table = torch.from_numpy(rng.normal(0., 0.1, (9, 3)).astype(np.float32)).to(dev)
    table[0] = 0.6
    table.requires_grad_(True)
    background = torch.tensor([0.1, 0.1, 0.2], device=dev, requires_grad=True)
    shapes = ((480, 640, 10, False), (2048, 2048, 16, False), (480, 640, 6, True), (2048, 2048, 6, True))
    if '--trace' in sys.argv:
        for h, w, c, tensor in shapes:
            g, col, d = inputs(dev, rng, h, w, c, tensor)
            for _ in range(3):     # the third dispatch of each kernel is the warm one
                fused_shader(g, col, table, background).backward(d)
                if not tensor:
                    one_light_shader(g).backward(d)
        torch.cuda.synchronize()
        return
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    steps = int(args[0]) if args else 10
    repeats = int(args[1]) if len(args) > 1 else 7
    out = {'steps': steps, 'repeats': repeats}
    for h, w, c, tensor in shapes:
        g, col, d = inputs(dev, rng, h, w, c, tensor)

        def leg(fn, g=g, col=col, d=d):
            def step():
                g.grad = table.grad = background.grad = None
                if col is not None:
                    col.grad = None
                fn(g, col, table, background).backward(d)
            return step

        r = time_alternating({'torch': leg(torch_shader), 'fused': leg(fused_shader)}, steps, repeats)
        r['speedup'] = r['torch']['ms'] / r['fused']['ms']
        r['faster_beyond_torch_spread'] = r['torch']['ms'] - r['fused']['ms'] > r['torch']['max'] - r['torch']['min']
        # bytes from shapes: forward reads the G-buffer (and the colours) and writes 3 channels; backward reads them and grad_out
        # and writes d gbuffer (and d colours)
        extra = 3 if tensor else 0
        r['fused_bytes'] = {'forward': 4 * h * w * (c + extra + 3), 'backward': 4 * h * w * (c + extra + 3 + c + extra)}
        r['fused_share_of_8TBps'] = sum(r['fused_bytes'].values()) / 8e12 / (r['fused']['ms'] * 1e-3)
        out['%s_%dx%dx%d' % ('tensor' if tensor else 'shader', w, h, c)] = r
        del g, col, d
    print(json.dumps(out))
    with open(os.path.join(ROOT, 'profiles', 'shade_sh.json'), 'w') as fh:
        json.dump({'note': 'MI355X; HIP events, legs alternating in one process, median [min, max] of %d blocks of %d steps '
                           '(tools/bench_shade_sh.py)' % (repeats, steps), 'bench_shade_sh': out}, fh, indent=1)


if __name__ == '__main__':
    main()
