"""The fused panorama resamplers (dirt_amd.texture.panorama_to_cube / cube_to_panorama) against the two routes available without
them.  Timed with HIP events after warm-up, in one process, the legs alternating (the method of tools/bench_shade.py), at
      to_cube_s1, to_cube_s2   a 1024 x 2048 x 3 panorama -> a 6 x 512 x 512 x 3 cube, samples 1 and 2;
      to_panorama_s1           a 6 x 512 x 512 x 3 cube -> a 512 x 1024 x 3 panorama, samples 1.
Legs:
      fused      the call, under a rotation;
      dense      the pure-torch specification (`panorama_to_cube_dense` / `cube_to_panorama_dense`), under the same rotation;
      composed   the cheapest route through the existing look-ups: the samples' (u, v) or directions computed ONCE, outside the
                 timed region, and fed to `sample_texture_uv(mode='repeat')` / `sample_texture_cube`, then reshape(...).mean.  With
                 its coordinates cached this leg does no trigonometry and can carry no gradient to a rotation: it does less than
                 the fused leg, not the same.  (Its panorama look-up also wraps rows and has no half-texel centre: it is there for
                 its cost, not its values.)
Per shape:
      forward                    the call alone, nothing requiring a gradient;
      forward_backward           forward + backward with the gradient to the sampled operand, which every leg can give;
      forward_backward_rotation  ... and to the rotation too: fused and dense only.
Every figure is the median over `repeats` blocks of `steps` steps, with the spread (min .. max) of the blocks.  The bar the README
uses for the word "faster": the fused leg's slowest block under the other leg's fastest; `fused_slowest_under_<leg>_fastest` says
whether it was.
usage (GPU box): python tools/bench_panorama.py [steps] [repeats]     (prints one JSON line, writes profiles/panorama.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from dirt_amd import matrices, texture  # noqa: E402
from bench_shade import time_alternating  # noqa: E402

CUBE, PANORAMA, OUT_PANORAMA = 512, (1024, 2048), (512, 1024)


def main():
    dev = torch.device('cuda', 0)
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    steps = int(args[0]) if args else 10
    repeats = int(args[1]) if len(args) > 1 else 7
    torch.manual_seed(0)
    rotation0 = matrices.rodrigues(torch.tensor([0.3, 0.5, 0.1]), three_by_three=True).to(dev)
    out = {'steps': steps, 'repeats': repeats}
    shapes = [('to_cube_s1', True, 1), ('to_cube_s2', True, 2), ('to_panorama_s1', False, 1)]
    for name, to_cube, S in shapes:
        rotation = rotation0.clone().requires_grad_(True)
        if to_cube:
            H, W = PANORAMA
            source = torch.rand(H, W, 3, device=dev).requires_grad_(True)
            d_out = torch.randn(6, CUBE, CUBE, 3, device=dev)
            with torch.no_grad():      # the composed leg's cached coordinates
                e = texture._rotate(texture._cube_sample_directions(CUBE, S, dev, torch.float32), rotation0, True)
                idx, _ = texture.directions_to_panorama_indices(e, H, W)
                uvs = torch.stack([idx[..., 1] / W, idx[..., 0] / H], -1).contiguous()
            fused = lambda: texture.panorama_to_cube(source, CUBE, samples=S, rotation=rotation)   # noqa: E731
            dense = lambda: texture.panorama_to_cube_dense(source, CUBE, S, rotation)   # noqa: E731
            composed = lambda: texture.sample_texture_uv(source, uvs, mode='repeat').reshape(6, CUBE, S, CUBE, S, 3).mean((2, 4))   # noqa: E731
            shape = {'panorama': [H, W, 3], 'cube': [6, CUBE, CUBE, 3], 'samples': S}
        else:
            H, W = OUT_PANORAMA
            source = torch.rand(6, CUBE, CUBE, 3, device=dev).requires_grad_(True)
            d_out = torch.randn(H, W, 3, device=dev)
            with torch.no_grad():
                dirs = texture._rotate(texture.panorama_texel_directions(H, W, S, dev)[0], rotation0, False).contiguous()
            fused = lambda: texture.cube_to_panorama(source, H, W, samples=S, rotation=rotation)   # noqa: E731
            dense = lambda: texture.cube_to_panorama_dense(source, H, W, S, rotation)   # noqa: E731
            composed = lambda: texture.sample_texture_cube(source, dirs).reshape(H, S, W, S, 3).mean((1, 3))   # noqa: E731
            shape = {'cube': [6, CUBE, CUBE, 3], 'panorama': [H, W, 3], 'samples': S}
        for mode in ('forward', 'forward_backward', 'forward_backward_rotation'):
            def leg(fn, mode=mode):
                def step():
                    if mode == 'forward':
                        with torch.no_grad():
                            fn()
                        return
                    source.grad = rotation.grad = None
                    rotation.requires_grad_(mode == 'forward_backward_rotation')
                    fn().backward(d_out)
                return step

            legs = {'dense': leg(dense), 'fused': leg(fused)}
            if mode != 'forward_backward_rotation':
                legs['composed'] = leg(composed)
            t = time_alternating(legs, steps, repeats)
            for other in legs:
                if other != 'fused':
                    t['fused_slowest_under_%s_fastest' % other] = t['fused']['max'] < t[other]['min']
            shape[mode] = t
        out[name] = shape
        del source, d_out
        torch.cuda.empty_cache()
    print(json.dumps(out))
    with open(os.path.join(ROOT, 'profiles', 'panorama.json'), 'w') as fh:
        json.dump({'note': 'MI355X; HIP events, legs alternating in one process, median [min, max] of %d blocks of %d steps; the composed leg '
                           'reads coordinates computed once outside the timed region and carries no gradient to a rotation '
                           '(tools/bench_panorama.py)' % (repeats, steps), 'bench_panorama': out}, fh, indent=1)


if __name__ == '__main__':
    main()
