"""The fused Cook-Torrance G-buffer lighting (dirt_amd.shading.shade_gbuffer_pbr) against the float32 torch composition of the
same shader (lighting.cook_torrance on slices of the G-buffer, the ambient term, the mask composite, the clamp), timed with
HIP events after warm-up, in one process, the two legs alternating (the method of tools/bench_shade.py):
  WxHxC_Llights   at 640x480x12 and 2048x2048x16 (mask, position, colour, normal, roughness, metalness; the rest unused), with
                  1 light (directional) and 4 lights (directional, point, point, directional):
      forward            the call alone, nothing requiring a gradient;
      forward_backward   forward + backward with gradients to the G-buffer and to every parameter (ambient, background,
                         camera, the lights' vectors and colours).
Every figure is the median over `repeats` blocks of `steps` steps, with the spread (min .. max) of the blocks.  No ratio is
required of this tool: it records what it reads.
usage (GPU box): python tools/bench_shade_pbr.py [steps] [repeats]     (prints one JSON line, writes profiles/shade_pbr.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from dirt_amd import lighting, shading  # noqa: E402
from bench_shade import time_alternating  # noqa: E402

LAYOUT = dict(mask=0, positions=1, colors=4, normals=7, material=10)
KINDS = ('directional', 'point', 'point', 'directional')


def torch_shader(gbuffer, lights, ambient, camera, background):
    m, p, c, n = gbuffer[..., :1], gbuffer[..., 1:4], gbuffer[..., 4:7], gbuffer[..., 7:10]
    lit = lighting.cook_torrance(p, n, c, gbuffer[..., 10], gbuffer[..., 11], camera, lights)
    return torch.clamp((ambient * c + lit) * m + background * (1. - m), 0., 1.)


def fused_shader(gbuffer, lights, ambient, camera, background):
    return shading.shade_gbuffer_pbr(gbuffer, lights, ambient=ambient, camera_position=camera, background=background, **LAYOUT)


def main():
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    steps = int(args[0]) if args else 10
    repeats = int(args[1]) if len(args) > 1 else 7
    t = lambda x: torch.tensor(x, dtype=torch.float32, device=dev, requires_grad=True)   # noqa: E731
    ambient, camera, background = t([0.1, 0.1, 0.1]), t([0.3, -0.2, 4.]), t([0., 0., 0.3])
    vectors = [t(v) for v in ([0.5, -0.6, -0.6], [-1.5, 2.5, 2.], [2., 1., 3.], [-0.3, -0.8, -0.5])]
    colors = [t(rng.uniform(0.2, 0.6, 3)) for _ in KINDS]
    out = {'steps': steps, 'repeats': repeats}
    for h, w, c in ((480, 640, 12), (2048, 2048, 16)):
        g = torch.rand(h, w, c, device=dev)
        g[..., 0] = (g[..., 0] < 0.7).float()
        g[..., 1:4] = g[..., 1:4] * 2. - 1.
        g[..., 7:10] = torch.nn.functional.normalize(g[..., 7:10] - 0.5, dim=-1)
        d = torch.from_numpy(rng.standard_normal((h, w, 3)).astype(np.float32)).to(dev)
        for count in (1, 4):
            lights = [(KINDS[i], vectors[i], colors[i]) for i in range(count)]
            params = [ambient, camera, background] + vectors[:count] + colors[:count]
            row = {}
            for name, leaf in (('forward', g.detach()), ('forward_backward', g.detach().requires_grad_(True))):
                def leg(fn, leaf=leaf, name=name, lights=lights, params=params):
                    def step():
                        if name == 'forward':
                            with torch.no_grad():
                                fn(leaf, lights, ambient, camera, background)
                            return
                        leaf.grad = None
                        for x in params:
                            x.grad = None
                        fn(leaf, lights, ambient, camera, background).backward(d)
                    return step

                r = time_alternating({'torch': leg(torch_shader), 'fused': leg(fused_shader)}, steps, repeats)
                r['speedup'] = r['torch']['ms'] / r['fused']['ms']
                row[name] = r
            # bytes from shapes: forward reads the G-buffer and writes 3 channels; backward reads it and grad_out and writes d gbuffer
            row['fused_bytes'] = {'forward': 4 * h * w * (c + 3), 'backward': 4 * h * w * (c + 3 + c)}
            row['fused_share_of_8TBps'] = sum(row['fused_bytes'].values()) / 8e12 / (row['forward_backward']['fused']['ms'] * 1e-3)
            out['%dx%dx%d_%dlights' % (w, h, c, count)] = row
        del g, d
    print(json.dumps(out))
    with open(os.path.join(ROOT, 'profiles', 'shade_pbr.json'), 'w') as fh:
        json.dump({'note': 'MI355X; HIP events, legs alternating in one process, median [min, max] of %d blocks of %d steps '
                           '(tools/bench_shade_pbr.py)' % (repeats, steps), 'bench_shade_pbr': out}, fh, indent=1)


if __name__ == '__main__':
    main()
