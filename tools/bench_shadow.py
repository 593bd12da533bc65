"""The fused shadow-map look-up (dirt_amd.shading.shadow_visibility) against the route available before it, the torch form
`lighting.shadow_visibility` on the same inputs.  Timed with HIP events after warm-up, in one process, the two legs alternating
(the method of tools/bench_shade.py), on a 1024 x 1024 x 10 G-buffer RENDERED from the scene of examples/fit_light_shadow_fused.py
(a box above a floor: neighbouring pixels look up neighbouring texels, as they do in use, so the backward's tiles have the boxes
they have in use) and 2048 x 2048 maps drawn by `render_shadow_map`, with L = 1 and 4 lights and kernel = 1 and 3:
      forward            the call alone, nothing requiring a gradient;
      forward_backward   forward + backward with gradients to the G-buffer, the maps and the matrices.
Every figure is the median over `repeats` blocks of `steps` steps, with the spread (min .. max) of the blocks.  Beside the times:
`bytes`, what a forward call must move, computed from the shapes -- per pixel the 12 bytes of the position, the 12 of the normal
(the normal offset is on), the 4 of the mask and 4 per light written, plus every map once -- and `share_of_8TBs`, those bytes
over the fused forward's time as a share of 8 TB/s.  The bar is that the fused call is faster than the torch form at each shape;
`fused_is_faster` says whether it was.
usage (GPU box): python tools/bench_shadow.py [steps] [repeats]     (prints one JSON line, writes profiles/shadow.json)"""
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import dirt_amd  # noqa: E402
from dirt_amd import lighting, shading  # noqa: E402
from bench_shade import time_alternating  # noqa: E402

LAYOUT = dict(mask=0, normals=4, positions=7)
DIRECTIONS = ([0.45, -0.8, -0.35], [-0.3, -0.9, 0.2], [0.1, -0.7, 0.6], [-0.5, -0.6, -0.4])


def torch_form(gbuffer, maps, matrices, *, positions, normals, mask, **kw):
    """`shadow_visibility` for a [H, W, Cg] G-buffer by `lighting.shadow_visibility` on its slices"""
    flat = gbuffer.reshape(-1, gbuffer.shape[-1])
    out = lighting.shadow_visibility(flat[:, positions:positions + 3], flat[:, normals:normals + 3], maps, matrices, mask=flat[:, mask], **kw)
    return out.reshape(tuple(gbuffer.shape[:-1]) + (maps.shape[0],))


def main():
    dev = torch.device('cuda', 0)
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    steps = int(args[0]) if args else 5
    repeats = int(args[1]) if len(args) > 1 else 5
    spec = importlib.util.spec_from_file_location('fit_light_shadow_fused', os.path.join(ROOT, 'examples', 'fit_light_shadow_fused.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    vertices, faces, normals, colors = (torch.from_numpy(a).to(dev) for a in ex.build_scene())
    h = w = 1024
    size = 2048
    with torch.no_grad():
        v4 = torch.cat([vertices, torch.ones_like(vertices[:, :1])], 1)
        attributes = torch.cat([torch.ones_like(vertices[:, :1]), colors, normals, vertices], 1)
        g = dirt_amd.rasterise(torch.zeros(h, w, 10, device=dev), v4 @ ex.camera_matrix(w, h, dev), attributes, faces).contiguous()
        all_matrices = torch.stack([ex.light_matrix(torch.tensor(d, device=dev)) for d in DIRECTIONS])
        all_maps = torch.stack([shading.render_shadow_map(vertices, faces, m, size, 1.) for m in all_matrices])
    d_out = torch.randn(h, w, len(DIRECTIONS), device=dev)
    out = {'steps': steps, 'repeats': repeats, 'gbuffer': [h, w, 10], 'map': [size, size], 'covered': float(g[..., 0].mean())}
    for lights in (1, 4):
        for kernel in (1, 3):
            kw = dict(kernel=kernel, bias=ex.BIAS, softness=ex.SOFTNESS, normal_offset=ex.NORMAL_OFFSET, **LAYOUT)
            maps, matrices = all_maps[:lights].clone().requires_grad_(True), all_matrices[:lights].clone().requires_grad_(True)
            d = d_out[..., :lights].contiguous()
            shape = {'bytes': h * w * (12 + 12 + 4 + 4 * lights) + lights * size * size * 4}
            for name, leaf in (('forward', g), ('forward_backward', g.clone().requires_grad_(True))):
                def leg(fn, leaf=leaf, name=name):
                    def step():
                        if name == 'forward':
                            with torch.no_grad():
                                fn(leaf, maps, matrices, **kw)
                            return
                        leaf.grad = maps.grad = matrices.grad = None
                        fn(leaf, maps, matrices, **kw).backward(d)
                    return step

                r = time_alternating({'torch': leg(torch_form), 'fused': leg(shading.shadow_visibility)}, steps, repeats)
                r['speedup'] = r['torch']['ms'] / r['fused']['ms']
                r['fused_is_faster'] = r['fused']['ms'] < r['torch']['ms']
                shape[name] = r
            shape['share_of_8TBs'] = shape['bytes'] / (shape['forward']['fused']['ms'] * 1e-3) / 8e12
            out['lights_%d_kernel_%d' % (lights, kernel)] = shape
    print(json.dumps(out))
    with open(os.path.join(ROOT, 'profiles', 'shadow.json'), 'w') as fh:
        json.dump({'note': 'MI355X; HIP events, legs alternating in one process, median [min, max] of %d blocks of %d steps '
                           '(tools/bench_shadow.py)' % (repeats, steps), 'bench_shadow': out}, fh, indent=1)


if __name__ == '__main__':
    main()
