"""Shadowed Cook-Torrance lighting of a G-buffer in one call (dirt_amd.shading.shade_gbuffer_pbr(..., visibility=)) against the
route composed of calls without the operand (DESIGN.md §7h before it): per light one `shade_gbuffer_pbr(gbuffer, [light_i],
ambient=0, background=0, clamp=None)` times `vis[..., i:i + 1]`, summed in torch, the ambient term and the background from one
more shader call, one `torch.clamp` -- only operations the library had before the operand.  The visibility is a resident
tensor [H, W, L] (the look-up that makes it is the same in both routes and is not timed).  HIP events after warm-up, in one
process, the two legs alternating in blocks (the method of tools/bench_shade.py):
  1024x1024x12_Llights   mask, position, colour, normal, roughness, metalness; L = 1, 2, 4 (directional, point, point, directional):
      forward            the call alone, nothing requiring a gradient;
      forward_backward   forward + backward with gradients to the G-buffer, the visibility and every parameter.
Every figure is the median over `repeats` blocks of `steps` steps, with the spread (min .. max) of the blocks.  The bar: at every
L the fused leg is faster by more than the spread between blocks of the same leg -- `separated`: the fused leg's slowest block is
faster than the composed leg's fastest.  The tool exits with status 1 where it is not.
usage (GPU box): python tools/bench_shade_pbr_visibility.py [steps] [repeats]     (prints one JSON line, writes
profiles/shade_pbr_visibility.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from dirt_amd import shading  # noqa: E402
from bench_shade import time_alternating  # noqa: E402

LAYOUT = dict(mask=0, positions=1, colors=4, normals=7, material=10)
KINDS = ('directional', 'point', 'point', 'directional')
ZERO = (0., 0., 0.)


def fused_shader(gbuffer, lights, visibility, ambient, camera, background):
    return shading.shade_gbuffer_pbr(gbuffer, lights, ambient=ambient, camera_position=camera, background=background, visibility=visibility,
                                     **LAYOUT)


def composed_shader(gbuffer, lights, visibility, ambient, camera, background):
    lit = shading.shade_gbuffer_pbr(gbuffer, [], ambient=ambient, camera_position=camera, background=background, clamp=None, **LAYOUT)
    for i, light in enumerate(lights):
        lit = lit + shading.shade_gbuffer_pbr(gbuffer, [light], ambient=ZERO, camera_position=camera, background=ZERO, clamp=None,
                                              **LAYOUT) * visibility[..., i:i + 1]
    return torch.clamp(lit, 0., 1.)


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
    h, w, c = 1024, 1024, 12
    g = torch.rand(h, w, c, device=dev)
    g[..., 0] = (g[..., 0] < 0.7).float()
    g[..., 1:4] = g[..., 1:4] * 2. - 1.
    g[..., 7:10] = torch.nn.functional.normalize(g[..., 7:10] - 0.5, dim=-1)
    d = torch.from_numpy(rng.standard_normal((h, w, 3)).astype(np.float32)).to(dev)
    out = {'steps': steps, 'repeats': repeats}
    for count in (1, 2, 4):
        lights = [(KINDS[i], vectors[i], colors[i]) for i in range(count)]
        params = [ambient, camera, background] + vectors[:count] + colors[:count]
        vis = torch.rand(h, w, count, device=dev)
        row = {}
        for name in ('forward', 'forward_backward'):
            grad = name == 'forward_backward'
            leaf, vleaf = g.detach().requires_grad_(grad), vis.detach().requires_grad_(grad)

            def leg(fn, leaf=leaf, vleaf=vleaf, grad=grad, lights=lights, params=params):
                def step():
                    if not grad:
                        with torch.no_grad():
                            fn(leaf, lights, vleaf, ambient, camera, background)
                        return
                    leaf.grad = vleaf.grad = None
                    for x in params:
                        x.grad = None
                    fn(leaf, lights, vleaf, ambient, camera, background).backward(d)
                return step

            r = time_alternating({'composed': leg(composed_shader), 'fused': leg(fused_shader)}, steps, repeats)
            r['speedup'] = r['composed']['ms'] / r['fused']['ms']
            r['separated'] = r['fused']['max'] < r['composed']['min']
            row[name] = r
        out['%dx%dx%d_%dlights' % (w, h, c, count)] = row
    out['bar_met'] = all(r[name]['separated'] for k, r in out.items() if isinstance(r, dict) for name in ('forward', 'forward_backward'))
    print(json.dumps(out))
    with open(os.path.join(ROOT, 'profiles', 'shade_pbr_visibility.json'), 'w') as fh:
        json.dump({'note': 'MI355X; HIP events, legs alternating in one process, median [min, max] of %d blocks of %d steps '
                           '(tools/bench_shade_pbr_visibility.py)' % (repeats, steps), 'bench_shade_pbr_visibility': out}, fh, indent=1)
    return 0 if out['bar_met'] else 1


if __name__ == '__main__':
    sys.exit(main())
