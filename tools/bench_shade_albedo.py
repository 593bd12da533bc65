"""The textured shader (examples/textured.py: a texture look-up lit by one diffuse light) with its lighting three ways, forward +
backward of the shader alone on a resident 6-channel G-buffer (mask, u, v, normal) and a 512 x 512 x 3 texture, gradients to the
texture, the G-buffer and the light direction; timed with HIP events after warm-up, in one process, the legs alternating:
  torch     the torch composition of examples/textured.py::shader_fn;
  cat       shade_gbuffer on torch.cat([gbuffer, unlit], -1) with colors=6: the fused lighting as it could be reached before;
  tensor    shade_gbuffer(gbuffer, colors=unlit): the colours read beside the G-buffer (examples/textured_fused.py::shader_fn).
The look-up (sample_texture_uv) is the same fused call in all three.  Every figure is the median over `repeats` blocks of `steps`
steps, with the spread (min .. max) of the blocks.
usage (GPU box): python tools/bench_shade_albedo.py [steps] [repeats] [--once]      (prints one JSON line; --once: one step of
each leg and no timing, for a kernel trace)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from dirt_amd import lighting, shading, texture as tex  # noqa: E402
from tools.bench_shade import time_alternating  # noqa: E402


def torch_shader(gbuffer, texture, light_direction):
    """examples/textured.py::shader_fn"""
    mask, uvs, normals = gbuffer[..., :1], gbuffer[..., 1:3], gbuffer[..., 3:]
    unlit = tex.sample_texture_uv(texture, uvs)
    diffuse = lighting.diffuse_directional(normals.reshape(-1, 3), unlit.reshape(-1, 3), light_direction,
                                           light_color=torch.full((3,), 0.6, device=gbuffer.device), double_sided=True)
    return (diffuse.reshape(unlit.shape) + unlit * 0.4) * mask + torch.tensor([0., 0., 0.3], device=gbuffer.device) * (1. - mask)


def _lit(gbuffer, light_direction, colors):
    return shading.shade_gbuffer(gbuffer, [shading.diffuse_directional_light(light_direction, (.6, .6, .6), True)], colors=colors, normals=3,
                                 mask=0, ambient=(.4, .4, .4), background=(0., 0., .3), clamp=None)


def cat_shader(gbuffer, texture, light_direction):
    return _lit(torch.cat([gbuffer, tex.sample_texture_uv(texture, gbuffer[..., 1:3])], -1), light_direction, 6)


def tensor_shader(gbuffer, texture, light_direction):
    return _lit(gbuffer, light_direction, tex.sample_texture_uv(texture, gbuffer[..., 1:3]))


LEGS = {'torch': torch_shader, 'cat': cat_shader, 'tensor': tensor_shader}


def frame(h, w, dev, rng):
    """a G-buffer as the textured cube rasterises it: 70 % covered, (u, v) smooth across the frame (two repeats), unit normals"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    n = rng.standard_normal((h, w, 3)).astype(np.float32)
    g = np.concatenate([(rng.uniform(size=(h, w, 1)) < 0.7).astype(np.float32), 2. * x[..., None] / w, 2. * y[..., None] / h,
                        n / np.linalg.norm(n, axis=-1, keepdims=True)], -1)
    return torch.from_numpy(g).to(dev).requires_grad_(True)


def main():
    numbers = [int(a) for a in sys.argv[1:] if not a.startswith('--')]
    steps, repeats = numbers[0] if numbers else 10, numbers[1] if len(numbers) > 1 else 7
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    texture = torch.from_numpy(rng.uniform(0., 1., (512, 512, 3)).astype(np.float32)).to(dev).requires_grad_(True)
    light = torch.nn.functional.normalize(torch.tensor([1., -0.3, -0.5], device=dev), dim=0).requires_grad_(True)
    out = {'steps': steps, 'repeats': repeats}
    for h, w in ((480, 640), (2048, 2048)):
        g = frame(h, w, dev, rng)
        d = torch.from_numpy(rng.standard_normal((h, w, 3)).astype(np.float32)).to(dev)

        def leg(fn, g=g, d=d):
            def step():
                g.grad = texture.grad = light.grad = None
                fn(g, texture, light).backward(d)
            return step

        if '--once' in sys.argv:
            for fn in LEGS.values():
                leg(fn)()
            torch.cuda.synchronize()
            continue
        r = time_alternating({k: leg(fn) for k, fn in LEGS.items()}, steps, repeats)
        r['tensor_over_cat'] = r['cat']['ms'] / r['tensor']['ms']
        r['tensor_over_torch'] = r['torch']['ms'] / r['tensor']['ms']
        # the condition: the new call is nowhere slower than the cat route beyond the cat route's own spread
        r['tensor_within_cat_spread'] = bool(r['tensor']['ms'] <= r['cat']['ms'] + (r['cat']['max'] - r['cat']['min']))
        # bytes of the lighting kernels, from shapes (forward: G-buffer and colours in, 3 channels out; backward: both and d out in,
        # d gbuffer and d colours out); the cat route reads and writes 9-channel rows and pays torch.cat and its backward besides
        px = 4 * h * w
        r['tensor_lighting_bytes'] = {'forward': px * (6 + 3 + 3), 'backward': px * (6 + 3 + 3 + 6 + 3)}
        r['cat_lighting_bytes'] = {'forward': px * (9 + 3), 'backward': px * (9 + 3 + 9), 'cat': px * (9 + 9), 'cat_backward': px * (9 + 9)}
        out['shader_%dx%d' % (w, h)] = r
        del g, d
    print(json.dumps(out))


if __name__ == '__main__':
    main()
