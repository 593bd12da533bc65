"""The fused G-buffer lighting (dirt_amd.shading.shade_gbuffer) against the torch shader it replaces (the composition of
examples/deferred.py::shader_fn), timed with HIP events after warm-up, in one process, the two legs alternating:
  shader_*      forward + backward of the shader alone on a resident G-buffer, at 640x480x10 and 2048x2048x16;
  deferred_*    rasterise_deferred forward + backward at K5 (2048x2048, 16 channels, 50 000 triangles) with each as its shader.
Every figure is the median over `repeats` blocks of `steps` steps, with the spread (min .. max) of the blocks.
usage (GPU box): python tools/bench_shade.py [steps] [repeats]        (prints one JSON line)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from dirt_amd import lighting, rasterise_ops as ops, shading  # noqa: E402
from tests import scenes  # noqa: E402

LAYOUT = dict(mask=0, positions=1, colors=4, normals=7)   # the sample's, inside 10 or 16 channels


def torch_shader(gbuffer, view_matrix, light_direction):
    """examples/deferred.py::shader_fn (samples/deferred.py:58-96) for a G-buffer of 10 or more channels"""
    mask, positions, unlit_colors, normals = gbuffer[..., :1], gbuffer[..., 1:4], gbuffer[..., 4:7], gbuffer[..., 7:10]
    dev = gbuffer.device
    ambient = unlit_colors * 0.2
    diffuse = lighting.diffuse_directional(normals.reshape(-1, 3), unlit_colors.reshape(-1, 3), light_direction,
                                           light_color=torch.tensor([1., 0., 0.], device=dev), double_sided=False)
    camera_position_world = torch.linalg.inv(view_matrix)[3, :3]
    specular = lighting.specular_directional(positions.reshape(-1, 3), normals.reshape(-1, 3), unlit_colors.reshape(-1, 3),
                                             light_direction, light_color=torch.tensor([1., 1., 1.], device=dev),
                                             camera_position=camera_position_world, shininess=6., double_sided=False)
    lit = diffuse.reshape(unlit_colors.shape) + specular.reshape(unlit_colors.shape) + ambient
    return torch.clamp(lit * mask + torch.tensor([0., 0., 0.3], device=dev) * (1. - mask), 0., 1.)


def fused_shader(gbuffer, view_matrix, light_direction):
    return shading.shade_gbuffer(
        gbuffer, [shading.diffuse_directional_light(light_direction, (1., 0., 0.), double_sided=False),
                  shading.specular_directional_light(light_direction, (1., 1., 1.), 6., double_sided=False)],
        ambient=(0.2, 0.2, 0.2), background=(0., 0., 0.3), camera_position=torch.linalg.inv(view_matrix)[3, :3], clamp=(0., 1.), **LAYOUT)


def time_alternating(legs, steps, repeats):
    """{name: fn} -> {name: {'ms', 'min', 'max'}}: blocks of `steps` calls between two HIP events, the legs taking turns"""
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / steps)
    return {k: {'ms': float(np.median(t)), 'min': min(t), 'max': max(t)} for k, t in times.items()}


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    view = torch.eye(4, device=dev)
    view[3, :3] = torch.tensor([0., -1.5, -3.5], device=dev)
    view.requires_grad_(True)
    light = torch.nn.functional.normalize(torch.tensor([1., -0.3, -0.5], device=dev), dim=0).requires_grad_(True)
    out = {'steps': steps, 'repeats': repeats}
    for h, w, c in ((480, 640, 10), (2048, 2048, 16)):
        g = torch.rand(h, w, c, device=dev)
        g[..., 0] = (g[..., 0] < 0.7).float()
        g.requires_grad_(True)
        d = torch.from_numpy(rng.standard_normal((h, w, 3)).astype(np.float32)).to(dev)

        def leg(fn, g=g, d=d):
            def step():
                g.grad = view.grad = light.grad = None
                fn(g, view, light).backward(d)
            return step

        r = time_alternating({'torch': leg(torch_shader), 'fused': leg(fused_shader)}, steps, repeats)
        r['speedup'] = r['torch']['ms'] / r['fused']['ms']
        # bytes from shapes: forward reads the G-buffer and writes 3 channels; backward reads both and writes d gbuffer
        nbytes = 4 * h * w * (c + 3 + c + 3 + c)
        r['fused_bytes'] = nbytes
        r['fused_share_of_8TBps'] = nbytes / 8e12 / (r['fused']['ms'] * 1e-3)
        out['shader_%dx%dx%d' % (w, h, c)] = r
        del g, d
    F, H, W, C, seed, r_lo, r_hi = scenes.CONFIGS['K5']
    s = scenes.rand_scene(F, H, W, C, seed, r_lo, r_hi)
    bg, v, a = (torch.from_numpy(s[k]).to(dev).requires_grad_(True) for k in ('background', 'vertices', 'vertex_colors'))
    f = torch.from_numpy(s['faces']).to(dev)
    d = torch.from_numpy(rng.standard_normal((H, W, 3)).astype(np.float32)).to(dev)

    def deferred(fn):
        def step():
            bg.grad = v.grad = a.grad = view.grad = light.grad = None
            ops.rasterise_deferred(bg, v, a, f, fn, [view, light]).backward(d)
        return step

    r = time_alternating({'torch': deferred(torch_shader), 'fused': deferred(fused_shader)}, max(1, steps // 2), repeats)
    r['speedup'] = r['torch']['ms'] / r['fused']['ms']
    out['deferred_K5'] = r
    print(json.dumps(out))


if __name__ == '__main__':
    main()
