"""The fused skybox (dirt_amd.shading.environment_background) against the route available before it, composed of four pieces:
`projection.unproject_pixels_to_rays` on a pixel grid built by hand -> `texture.sample_texture_cube` on the [H, W, 3] ray image
-> (1 - m) * intensity * E.  Timed with HIP events after warm-up, in one process, the two legs alternating (the method of
tools/bench_shade.py), at 1024 x 1024 and 640 x 480 pixels behind a 6 x 512 x 512 x 3 cube, with
      bilinear    both legs;
      trilinear   the fused leg at the level of detail of each pixel's analytic footprint; the composed leg at a CONSTANT lod
                  (a tensor of 0.5): it has no footprint form -- `sample_texture_cube` refuses a trilinear call without lod --
                  so it does less work per pixel than the fused leg, not the same;
and with two masks: none (every pixel is background) and the sphere of examples/fit_environment_background_fused.py (a disc of a
third of the image's height in radius: the share of the image that example's mesh covers).  Per shape:
      forward            the call alone, nothing requiring a gradient;
      forward_backward   forward + backward with gradients to the cube, the matrix and the intensity.
Every figure is the median over `repeats` blocks of `steps` steps, with the spread (min .. max) of the blocks.  Beside the times:
`bytes`, what a forward call must move, computed from the shapes -- per pixel the 12 bytes written and the 4 of the mask where
there is one, plus every texel of level 0 the image can reach once, bounded by the whole cube -- and `share_of_8TBs`, those bytes
over the fused forward's time as a share of 8 TB/s.  The bar: the fused leg's slowest block under the composed leg's fastest, at
each shape, forward and forward + backward; `fused_slowest_under_composed_fastest` says whether it was.
usage (GPU box): python tools/bench_background.py [steps] [repeats]     (prints one JSON line, writes profiles/background.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from dirt_amd import matrices, projection, shading, texture  # noqa: E402
from bench_shade import time_alternating  # noqa: E402

CUBE = 512
INTENSITY = (0.9, 1.0, 1.1)


def composed(cube, clip_to_world, size, mask, intensity, filter, lod):
    """the route a user had: the pixel grid, the rays, the look-up, the composite"""
    height, width = size
    cols, rows = torch.meshgrid(torch.arange(width, device=cube.device) + 0.5, torch.arange(height, device=cube.device) + 0.5, indexing='xy')
    directions = projection.unproject_pixels_to_rays(torch.stack([cols, rows], -1), clip_to_world, torch.tensor([width, height], device=cube.device))[1]
    looked = texture.sample_texture_cube(cube, directions, filter=filter, **({'lod': lod} if filter == 'trilinear' else {}))
    scale = intensity if mask is None else (1. - mask)[..., None] * intensity
    return scale * looked


def main():
    dev = torch.device('cuda', 0)
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    steps = int(args[0]) if args else 10
    repeats = int(args[1]) if len(args) > 1 else 7
    torch.manual_seed(0)
    out = {'steps': steps, 'repeats': repeats, 'cube': [6, CUBE, CUBE, 3]}
    for height, width in ((1024, 1024), (480, 640)):
        view = matrices.compose(matrices.rodrigues(torch.tensor([0.3, 0.5, 0.1])), matrices.translation(torch.tensor([0., 0., -3.])))
        proj = matrices.perspective_projection(near=0.1, far=20., right=0.05, aspect=float(height) / width)
        inverse = torch.linalg.inv((view @ proj).double()).float().to(dev)
        r, c = torch.meshgrid(torch.arange(height, device=dev) - height / 2., torch.arange(width, device=dev) - width / 2., indexing='ij')
        sphere = ((r * r + c * c) < (height / 3.) ** 2).float()
        d_out = torch.randn(height, width, 3, device=dev)
        lod = torch.full((height, width), 0.5, device=dev)
        for filter in ('bilinear', 'trilinear'):
            for mask_name, mask in (('background', None), ('sphere', sphere)):
                cube = torch.rand(6, CUBE, CUBE, 3, device=dev).requires_grad_(True)
                M = inverse.clone().requires_grad_(True)
                intensity = torch.tensor(INTENSITY, device=dev).requires_grad_(True)
                pixels = height * width
                shape = {'covered': 0. if mask is None else float(mask.mean()),
                         'bytes': pixels * (12 + (0 if mask is None else 4)) + min(6 * CUBE * CUBE, 4 * pixels) * 12}

                def fused_call():
                    return shading.environment_background(cube, M, (height, width), mask=mask, intensity=intensity, filter=filter)

                def composed_call():
                    return composed(cube, M, (height, width), mask, intensity, filter, lod)

                for name in ('forward', 'forward_backward'):
                    def leg(fn, name=name):
                        def step():
                            if name == 'forward':
                                with torch.no_grad():
                                    fn()
                                return
                            cube.grad = M.grad = intensity.grad = None
                            fn().backward(d_out)
                        return step

                    t = time_alternating({'composed': leg(composed_call), 'fused': leg(fused_call)}, steps, repeats)
                    t['speedup'] = t['composed']['ms'] / t['fused']['ms']
                    t['fused_slowest_under_composed_fastest'] = t['fused']['max'] < t['composed']['min']
                    shape[name] = t
                shape['share_of_8TBs'] = shape['bytes'] / (shape['forward']['fused']['ms'] * 1e-3) / 8e12
                out['%dx%d_%s_%s' % (height, width, filter, mask_name)] = shape
    print(json.dumps(out))
    with open(os.path.join(ROOT, 'profiles', 'background.json'), 'w') as fh:
        json.dump({'note': 'MI355X; HIP events, legs alternating in one process, median [min, max] of %d blocks of %d steps; the composed '
                           'trilinear leg reads a constant lod of 0.5, the fused one the footprint of each pixel (tools/bench_background.py)'
                           % (repeats, steps), 'bench_background': out}, fh, indent=1)


if __name__ == '__main__':
    main()
